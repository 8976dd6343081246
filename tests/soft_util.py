"""The oracle of soft (likelihood) evidence (nipamd_fb_soft,
nipamd_filter_soft): textbook_util.smoother with the step evidence
generalised, in plain numpy over an interface chain's own tables, vectorised
over sequences.

  e_t[y] = prod_hard E_k[y][o_{k,t}]  prod_soft sum_o w_{k,t}[o] E_k[y][o]

A hard column follows viterbi_util.evidence (-1 missing: the row sum; out of
range: zero); a soft column is a [B, T, M] weight array entering as w @ E.T.
A weight that is negative, NaN or infinite leaves its step without evidence.

The results do not depend on a vector's scale: every soft vector is used as
w 2^-k, k the exponent of its largest valid weight (np.frexp / np.ldexp: exact,
denormal weights included), and k ln 2 goes to that step's ll term.  So c w
gives the rows of w and adds log c to ll for every c that keeps the weights
finite, each factor of e_t is of the size of its table's entries, and a step is
without mass only where its evidence is truly zero: an all-zero vector, a bad
weight, no overlap with the states the chain can be in -- never by underflow
or overflow of the weights.

A sequence whose step mass is zero at step d is dead from there on: ll =
-DBL_MAX, all smoothed rows zero, the filtered rows zero from d on; its status
is 1, plus 4 when a bad weight was met (the streams' definition,
include/nip_amd.h).  tests/test_soft_api.py pins this oracle to
textbook_util.smoother and, at every weight scale, to a wide-exponent
evaluation of the same recursion.
"""
import numpy as np

from stream_util import digit_sums  # noqa: F401  (the joint interface's marginals, for the callers)
from viterbi_util import DBL_MAX, LN2, evidence

HARD, SOFT = "hard", "soft"


def step_evidence(Es, kinds, cols, liks, t):
    """(e_t [B, N], bad [B], k [B]): the step's evidence with every soft vector
    at the scale of its largest valid weight, whether a weight of step t is
    bad, and the sum of the exponents taken out (e_t 2^k is the evidence of the
    weights as given).
    kinds[k]: HARD -- cols[k] is a [B, T] int array -- or SOFT -- liks[k] is a
    [B, T, M_k] float array (the other list's entry is ignored)."""
    hard = [(E, c) for E, kind, c in zip(Es, kinds, cols) if kind == HARD]
    B = next(c.shape[0] for kind, c in zip(kinds, cols) if kind == HARD) if hard else \
        next(w.shape[0] for kind, w in zip(kinds, liks) if kind == SOFT)
    N = Es[0].shape[0]
    e = evidence([E for E, _ in hard], [c for _, c in hard], t) if hard else np.ones((B, N))
    bad = np.zeros(B, bool)
    ksum = np.zeros(B, np.int64)
    for E, kind, w in zip(Es, kinds, liks):
        if kind != SOFT:
            continue
        wt = np.asarray(w[:, t], np.float64)
        wb = ~(np.isfinite(wt) & (wt >= 0.0))
        bad |= wb.any(axis=1)
        wt = np.where(wb, 0.0, wt)
        _, k = np.frexp(wt.max(axis=1))                     # 0 for a maximum of 0
        ksum += k
        e = e * (np.ldexp(wt, -k[:, None]) @ E.T)
    e[bad] = 0.0
    return e, bad, ksum


def soft_smoother(A, pi, Es, kinds, cols, liks):
    """Returns (smoothed [B, T, N], filtered [B, T, N], ll [B]); soft_status
    gives the status words of the same request."""
    smoothed, filtered, ll, _ = _run(A, pi, Es, kinds, cols, liks)
    return smoothed, filtered, ll


def soft_status(A, pi, Es, kinds, cols, liks):
    return _run(A, pi, Es, kinds, cols, liks)[3]


def _run(A, pi, Es, kinds, cols, liks):
    T = next(c.shape[1] for kind, c in zip(kinds, cols) if kind == HARD) if HARD in kinds else \
        next(w.shape[1] for kind, w in zip(kinds, liks) if kind == SOFT)
    N = A.shape[0]
    s_all = np.ones(N)
    for E in Es:
        s_all = s_all * E.sum(axis=1)
    ev = [step_evidence(Es, kinds, cols, liks, t) for t in range(T)]
    B = ev[0][0].shape[0]
    ah = np.zeros((B, T, N))
    ll = np.zeros(B)
    ksum = np.zeros(B, np.int64)                            # the exponents taken out of the weights
    status = np.zeros(B, np.int64)
    alive = np.ones(B, bool)
    prev = np.tile(pi, (B, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(T):
            e, bad, k = ev[t]
            status[bad] |= 4
            u = prev @ A
            al = u * e
            c = al.sum(axis=1)
            alive &= c > 0.0
            ll += np.where(alive, np.log(c) - np.log((u * s_all).sum(axis=1)), 0.0)
            ksum += k
            prev = np.where(alive[:, None], al / c[:, None], 0.0)
            ah[:, t] = prev
        ll = ll + ksum * LN2
        status[~alive] |= 1
        ll[~alive] = -DBL_MAX
        post = np.empty_like(ah)
        post[:, T - 1] = ah[:, T - 1]
        b = np.ones((B, N))
        for t in range(T - 2, -1, -1):
            b = (ev[t + 1][0] * b) @ A.T
            b = np.where(alive[:, None], b / b.sum(axis=1, keepdims=True), 0.0)
            p = ah[:, t] * b
            post[:, t] = p / p.sum(axis=1, keepdims=True)
        post[~alive] = 0.0
    return post, ah, ll, status
