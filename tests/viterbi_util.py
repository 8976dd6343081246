"""A plain numpy Viterbi over an interface chain, vectorised over sequences
(fp64), built from a compiled model's own tables (textbook_util.chain_tables)
-- the oracle of most_likely_states; the reference declares mlss and never
implemented it, so there is nothing else to compare with.

  u0[y]      = sum_x pi[x] A[x][y]                 (slice -1 is summed out)
  e_t[y]     = prod_k E_k[y][m_k,t]                (the row sum for a missing value, 0 for a state out of range)
  delta_0    = u0 o e_0
  delta_t[y] = (max_x delta_{t-1}[x] A[x][y]) e_t[y],  psi_t[y] = the lowest x attaining the max
  x*_{T-1}   = the lowest argmax_y delta_{T-1}[y],  x*_{t-1} = psi_t[x*_t]
  logp       = ln max_y delta_{T-1}[y]

in the probability domain, each step's delta rescaled by the power of two of
its maximum (frexp / ldexp: exact, changes no comparison) with the exponents
carried into logp.  Es holds every child of the interface; a child nothing
observes gets a column of -1.
"""
import itertools

import numpy as np

DBL_MAX = np.finfo(np.float64).max
LN2 = float(np.log(2.0))


def evidence(Es, cols, t):
    """e_t [B, N]; cols: one [B, T] int array per table of Es."""
    B = cols[0].shape[0] if cols else 1
    N = Es[0].shape[0] if Es else 0
    e = np.ones((B, N))
    for E, c in zip(Es, cols):
        x = c[:, t]
        M = E.shape[1]
        ee = E[:, np.clip(x, 0, M - 1)].T.copy()
        ee[x < 0] = E.sum(axis=1)
        ee[x >= M] = 0.0
        e = e * ee
    return e


def viterbi(A, pi, Es, cols, B=None, T=None):
    """path [B, T] (-1 where a sequence has no mass), logp [B] (-DBL_MAX there)."""
    if cols:
        B, T = cols[0].shape
    N = A.shape[0]
    ev = (lambda t: evidence(Es, cols, t)) if cols else (lambda t: np.ones((B, N)))
    d = (pi @ A)[None, :] * ev(0)
    esum = np.zeros(B)
    psi = np.zeros((B, T, N), np.int64)
    for t in range(1, T):
        _, ex = np.frexp(d.max(axis=1))
        d = np.ldexp(d, -ex[:, None])
        esum += ex
        p = d[:, :, None] * A[None, :, :]                   # [B, x, y]
        psi[:, t] = p.argmax(axis=1)                        # numpy: the lowest index
        d = p.max(axis=1) * ev(t)
    m = d.max(axis=1)
    dead = ~(m > 0)
    path = np.zeros((B, T), np.int64)
    path[:, T - 1] = d.argmax(axis=1)
    rows = np.arange(B)
    for t in range(T - 1, 0, -1):
        path[:, t - 1] = psi[rows, t, path[:, t]]
    with np.errstate(divide="ignore"):
        logp = np.where(dead, -DBL_MAX, np.log(np.where(dead, 1.0, m)) + esum * LN2)
    path[dead] = -1
    return path, logp


def path_score(A, pi, Es, cols, path):
    """ln of the measure of (path, evidence) per sequence: the sum of the log
    terms of a given path [B, T]; -inf where a term is 0."""
    B, T = path.shape
    rows = np.arange(B)
    ev = (lambda t: evidence(Es, cols, t)) if cols else (lambda t: np.ones((B, A.shape[0])))
    with np.errstate(divide="ignore"):
        s = np.log((pi @ A)[path[:, 0]]) + np.log(ev(0)[rows, path[:, 0]])
        for t in range(1, T):
            s = s + np.log(A[path[:, t - 1], path[:, t]]) + np.log(ev(t)[rows, path[:, t]])
    return s


def brute_force(A, pi, Es, cols_b):
    """One sequence (cols_b: one [T] array per table): the maximum of
    path_score over all N^T paths, and the lexicographically lowest
    maximiser."""
    T = cols_b[0].shape[0]
    N = A.shape[0]
    paths = np.array(list(itertools.product(range(N), repeat=T)), np.int64)
    cols = [np.tile(c[None, :], (paths.shape[0], 1)) for c in cols_b]
    s = path_score(A, pi, Es, cols, paths)
    k = int(s.argmax())
    return float(s[k]), paths[k]


def joint_tables(m, prev, cur, child):
    """Joint-interface chain tables by einsum over the product of every
    clique's table (the slice's joint): A [K, K], pi [K], E [K, M] with the
    joint state's first variable fastest (prev / cur paired by position),
    child the one observed leaf of the interface."""
    import nip_amd
    from textbook_util import clique_vars
    nc = nip_amd.lib().nipamd_model_num_cliques(m._h)
    letters = "abcdefghijklmnop"
    ops, subs = [], []
    for c in range(nc):
        cv = clique_vars(m, c)
        ops.append(m.original(c).reshape([m.card(v) for v in reversed(cv)]))
        subs.append("".join(letters[v] for v in reversed(cv)))
    out = list(reversed(prev)) + list(reversed(cur)) + [child]
    F = np.einsum(",".join(subs) + "->" + "".join(letters[v] for v in out), *ops)
    K = int(np.prod([m.card(v) for v in cur]))
    F = F.reshape(K, K, m.card(child))                       # C order: the last variable of prev / cur slowest
    A = F.sum(axis=2)
    E = F.sum(axis=0) / A.sum(axis=0)[:, None]
    pi = np.ones(1)
    for v in prev:                                           # first variable fastest
        pi = np.kron(np.asarray(m.prior(v)), pi)
    return A, pi, E
