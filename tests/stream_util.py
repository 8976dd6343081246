"""The oracle of online inference (nip_amd.Stream): fixed-lag smoothing in
plain numpy over an interface chain's own tables (textbook_util.chain_tables,
viterbi_util.joint_tables), vectorised over sequences.

  row t = P(x_t | y_0 .. y_{min(t + L, T - 1)})
        = normalise(alpha^_t o beta),  beta = 1 at the endpoint,
          beta <- A (e_j o beta) for j = endpoint .. t + 1

The filtered alpha^ and the ll are textbook_util.smoother's forward pass,
computed once; every row then runs its own <= L backward steps.  L = 0 gives
the filtered rows, L >= T - 1 the smoothed ones (pinned to smoother run on
each prefix by tests/test_stream_api.py).
"""
import numpy as np

from textbook_util import smoother
from viterbi_util import evidence


def fixed_lag(A, pi, Es, cols, L):
    """cols: one [B, T] int array per table of Es (-1 missing).  Returns the
    fixed-lag rows [B, T, N] and the ll [B] of all T steps."""
    _, ah, ll = smoother(A, pi, Es, cols)
    B, T, N = ah.shape
    ev = [evidence(Es, cols, t) for t in range(T)]
    rows = np.empty_like(ah)
    for t in range(T):
        b = np.ones((B, N))
        for j in range(min(t + L, T - 1), t, -1):
            b = (ev[j] * b) @ A.T
            b = b / b.sum(axis=1, keepdims=True)
        p = ah[:, t] * b
        rows[:, t] = p / p.sum(axis=1, keepdims=True)
    return rows, ll


def digit_sums(rows, stride, card):
    """Marginal of one variable of a joint interface: rows [..., K] over the
    joint state (the first variable fastest) summed into digit
    (state // stride) % card."""
    K = rows.shape[-1]
    out = np.zeros(rows.shape[:-1] + (card,))
    for x in range(K):
        out[..., (x // stride) % card] += rows[..., x]
    return out


def sticky_tables(N, M, seed):
    """A chain that remembers: A = 0.97 I + 0.03 R (R random row-stochastic) and
    emission rows 1 + 0.3 (u - 1/2), normalised -- dense random tables forget
    within a dozen steps, and lag 16 could not be told from lag 17 on them."""
    rng = np.random.default_rng(seed)
    R = rng.random((N, N))
    R /= R.sum(axis=1, keepdims=True)
    A = 0.97 * np.eye(N) + 0.03 * R
    E = 1.0 + 0.3 * (rng.random((N, M)) - 0.5)
    E /= E.sum(axis=1, keepdims=True)
    pi = rng.random(N) + 0.5
    pi /= pi.sum()
    return A, pi, E


def sticky_spec(N, M, seed):
    """sticky_tables as a model spec in synth.hmm_spec(proper=True)'s
    declaration order (child first: the parser's re-normalisation then runs
    over each family's child and leaves these rows as written).  CPT data is
    child-fastest, one row per parent state."""
    A, pi, E = sticky_tables(N, M, seed)
    nodes = [("M1", M, None), ("P1", N, None), ("P0", N, "P1")]
    pots = [("M1", ["P1"], E.ravel()), ("P1", ["P0"], A.ravel()), ("P0", [], pi)]
    return nodes, pots
