"""The oracle of the e_step under soft evidence (nipamd_estep_soft_partial,
nipamd_estep_soft): soft_util._run extended to the wide slab's three sums, per
sequence, in plain numpy over an interface chain's own tables.

With alpha^_t, beta_t and e_t as in soft_util (every soft vector at the scale
of its largest valid weight), every step normalised on its own as
textbook_util.chain_sums_torch does:

  K[x][y]   += alpha^_{t-1}[x] e_t[y] beta_t[y] / Z_t      (alpha^_{-1} = prior, no transition factor)
  P0[x]      = prior[x] (A (e_0 o beta_0))[x] / Z_0
  H_k[r][y] += gamma_t[y]                  child k hard: r its code's row (states, missing, out of range)
  H_k[o][y] += gamma_t[y] w[o] E_k[y][o] / sum_o' w[o'] E_k[y][o']      child k soft (0 where the sum is 0)

A plan child that no column names is a HARD column of -1.  A dead sequence
(soft_util's: no mass at some step) has ll = -DBL_MAX, status 1 | 2 (| 4 for a
bad weight) and all-zero sums.

star_counts projects the sums of a star model (the interface variable and its
leaf children, no hidden parents) onto the em_learn layout, as
nipamd_estep_finalize does: P0; A o K at y + N x; each child's H[o][y] plus its
missing row split as E[y][o] / s[y], at o + M y; the families in variable
order.  tests/test_estep_soft_api.py pins all of this to
textbook_util.hmm_estep_torch at one-hot and all-ones weights.
"""
import numpy as np

import soft_util as so
from soft_util import HARD, SOFT


def soft_sums(A, pi, Es, kinds, cols, liks):
    """Per sequence: (K [B, N, N], Hs -- one [B, M_k + 2, N] per child --, P0
    [B, N], ll [B], status [B]).  Arguments as soft_util.soft_smoother."""
    _, ah, ll, status = so._run(A, pi, Es, kinds, cols, liks)
    B, T, N = ah.shape
    ev = [so.step_evidence(Es, kinds, cols, liks, t)[0] for t in range(T)]
    dead = (status & 1) != 0
    status = status | np.where(dead, 3, 0)
    K = np.zeros((B, N, N))
    Hs = [np.zeros((B, E.shape[1] + 2, N)) for E in Es]
    P0 = np.zeros((B, N))
    b = np.ones((B, N))
    rows = np.arange(B)
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(T - 1, -1, -1):
            if t < T - 1:
                b = (ev[t + 1] * b) @ A.T
                b = b / b.sum(axis=1, keepdims=True)
            w = ev[t] * b
            pv = ah[:, t - 1] if t > 0 else np.tile(pi, (B, 1))
            n = ((pv @ A) * w).sum(axis=1)
            K += (pv / n[:, None])[:, :, None] * w[:, None, :]
            g = ah[:, t] * b
            g = g / g.sum(axis=1, keepdims=True)
            for H, E, kind, c, lk in zip(Hs, Es, kinds, cols, liks):
                M = E.shape[1]
                if kind == HARD:
                    r = c[:, t]
                    r = np.where(r < 0, M, np.where(r >= M, M + 1, r))
                    H[rows, r] += g
                else:
                    wt = np.asarray(lk[:, t], np.float64)
                    wt = np.where(np.isfinite(wt) & (wt >= 0.0), wt, 0.0)
                    _, k = np.frexp(wt.max(axis=1))
                    num = np.ldexp(wt, -k[:, None])[:, :, None] * E.T[None, :, :]     # [B, M, N]
                    den = num.sum(axis=1, keepdims=True)
                    H[:, :M] += np.where(den > 0.0, g[:, None, :] * (num / den), 0.0)
            if t == 0:
                g0 = pi[None, :] * (w @ A.T)
                P0 = g0 / g0.sum(axis=1, keepdims=True)
    K[dead] = 0.0
    P0[dead] = 0.0
    for H in Hs:
        H[dead] = 0.0
    return K, Hs, P0, ll, status


def slab(N, K, Hs, P0):
    """The sums over the sequences in the wide slab's layout: K [NP][NP], the
    children's H rows concatenated [R][NP], P0 [NP], NP = 16, 32 or 64."""
    NP = 16 if N <= 16 else 32 if N <= 32 else 64
    k = np.zeros((NP, NP))
    k[:N, :N] = K.sum(axis=0)
    h = np.zeros((sum(H.shape[1] for H in Hs), NP))
    h[:, :N] = np.concatenate([H.sum(axis=0) for H in Hs], axis=0)
    p = np.zeros(NP)
    p[:N] = P0.sum(axis=0)
    return np.concatenate([k.ravel(), h.ravel(), p])


def star_blocks(A, Es, K, Hs, P0):
    """The em_learn families of a star model from the sums over the sequences:
    (P0 [N], the interface's [N N] at y + N x, one [M N] per child at o + M y)."""
    trans = (A * K.sum(axis=0)).ravel()
    kids = []
    for E, H in zip(Es, Hs):
        M = E.shape[1]
        Hsum = H.sum(axis=0)                                    # [M + 2, N]
        s = E.sum(axis=1)
        share = np.divide(E, s[:, None], out=np.zeros_like(E), where=s[:, None] != 0.0)   # [N, M]
        kids.append((Hsum[:M].T + Hsum[M][:, None] * share).ravel())
    return P0.sum(axis=0), trans, kids


def star_counts(m, prev, cur, children, A, Es, K, Hs, P0, pseudo=1.0):
    """The counts e_step_soft gives for a star model m (variable indices prev,
    cur, children): star_blocks at the families' offsets in variable order, on
    top of the pseudo-counts."""
    p0, trans, kids = star_blocks(A, Es, K, Hs, P0)
    blocks = dict(zip([prev, cur] + list(children), [p0, trans] + kids))
    assert sorted(blocks) == list(range(m.num_vars)), "a star model: the interface and its leaf children"
    return pseudo + np.concatenate([blocks[v] for v in sorted(blocks)])


def one_hot(codes, M):
    """Likelihood vectors of hard codes [B, T]: one-hot, all ones where missing."""
    return np.where((codes < 0)[:, :, None], 1.0, np.eye(M)[np.maximum(codes, 0)])
