"""Soft evidence at every weight scale: the models, weights and scale patterns
of tests/test_gpu_soft_scale.py, which tests/test_soft_api.py evaluates with
its wide-exponent reference on a machine without a GPU.

A request (Req) names a builder of tests/test_gpu_soft.py -- the smallest shape
that reaches each path of chain_soft_kernel -- and which of its columns are
soft.  Base weights are 0.05 + U[0, 1); a pattern multiplies every step's
vector of every soft column by 2^k (np.ldexp: exact), one pattern per sequence
of a batch of B = 7:

  0   the control, k = 0
  1   k = -big on every column at t = 5..12
  2   k = -big on every column at every step
  3   k = +big at even steps, -big at odd ones, on every column
  4   k = +340 on every column at every step
  5   opposite signs on different columns: (+900, -900); from three columns on
      (-450, -450, +900, 0); a single column +900
  6   k random in [-900, 900] per step and column

with big = 560 (2^-560 = 2.6e-169: the product of two columns is 0 in fp64,
that of two columns at +560 is inf) or 530 (2^-530 = 2.8e-160: the product of
two columns is a denormal with about three digits).  At +340 the product of
two columns is 2^680 and still finite, that of four is not; two columns
overflow at the even steps of pattern 3.

The edge batch (edge_weights) is not an exact rescaling of the base weights
and is checked against the oracle only:

  0   the control
  1   every vector: entries multiplied by 2^-U{0..600}, one entry left as it is
  2   the same at the odd steps only
  3   every vector all denormal: w 2^-1070
  4   all denormal at t = 5..12
  5   the first column's vector is [DBL_MAX, DBL_MAX, ...] at every step
  6   the last column's vector is [DBL_MAX, ...] at t = 5..12
"""
import collections

import numpy as np

import stream_util as su
from soft_util import HARD, SOFT

B = 7
TS = (24, 37)
DBL_MAX = np.finfo(np.float64).max

# builder: a function of test_gpu_soft; soft: the soft columns' indices among
# the tables; hard: the hard columns' (observed codes, 20 % missing); the other
# tables' columns are missing throughout.  digits: the queried variables of a
# joint interface as (stride, card) digit sums of the joint row, in query order.
Req = collections.namedtuple("Req", "name m tables soft hard sv ov q digits")


def requests():
    """name -> Req, the models built once (test_gpu_soft caches them; importing
    it takes torch, its builders no GPU)."""
    import test_gpu_soft as tg
    out = {}

    def add(name, m, tables, soft, hard, kids, q, digits=None):
        out[name] = Req(name, m, tables, tuple(soft), tuple(hard), [kids[k] for k in soft],
                        [kids[k] for k in hard], q, digits)

    for name, args in (("hmm16", (16, 16, False)), ("hmm16-proper", (16, 16, True)), ("hmm3x20-long", (3, 20, False))):
        m, P1, M1, tables = tg.hmm(*args)
        add(name, m, tables, [0], [], [M1], [P1])
    m, v, tables = tg.demo1(20)
    add("demo20-both", m, tables, [0, 1], [], [v["A1"], v["B1"]], [v["C1"]])
    add("demo20-a-soft-b-hard", m, tables, [0], [1], [v["A1"], v["B1"]], [v["C1"]])
    m, X1, O1, tables = tg.wide()
    add("wide64", m, tables, [0], [], [O1], [X1])
    m, P1, ov, tables = tg.five_children()
    add("five-children-4-soft", m, tables, [0, 1, 2, 3], [], ov, [P1])
    m, cur, O1, tables = tg.factorial()
    X1, Y1 = m.variable("X1"), m.variable("Y1")
    stride = {cur[0]: 1, cur[1]: m.card(cur[0])}
    add("factorial-yx", m, tables, [0], [], [O1], [Y1, X1], [(stride[Y1], 4), (stride[X1], 4)])
    return out


NAMES = ["hmm16", "hmm16-proper", "hmm3x20-long", "demo20-both", "demo20-a-soft-b-hard", "wide64",
         "five-children-4-soft", "factorial-yx"]
TWO_COLUMN = ["demo20-both", "demo20-a-soft-b-hard"]


def cards(r, which):
    return [r.tables[2][k].shape[1] for k in which]


def base_weights(r, T, seed=0):
    """One [B, T, M] array per soft column, 0.05 + U[0, 1)."""
    rng = np.random.default_rng(4000 + 10 * T + len(r.soft) + seed)
    return [0.05 + rng.random((B, T, c)) for c in cards(r, r.soft)]


def hard_obs(r, T):
    """int32 [B, T, n_hard], 20 % missing."""
    rng = np.random.default_rng(5000 + T)
    cs = cards(r, r.hard)
    obs = np.stack([rng.integers(0, c, size=(B, T)) for c in cs], axis=2).astype(np.int32) if cs \
        else np.zeros((B, T, 0), np.int32)
    obs[rng.random(obs.shape) < 0.2] = -1
    return obs


def exponents(T, ncol, big=560):
    """k [B, T, ncol] of the patterns above."""
    k = np.zeros((B, T, ncol), np.int64)
    t = np.arange(T)
    k[1, 5:13] = -big
    k[2] = -big
    k[3] = np.where(t % 2 == 0, big, -big)[:, None]
    k[4] = 340
    k[5] = ([900], [900, -900], [-450, -450, 900], [-450, -450, 900, 0])[ncol - 1]
    k[6] = np.random.default_rng(6000 + 10 * T + ncol).integers(-900, 901, size=(T, ncol))
    return k


def scaled(liks, k):
    return [np.ldexp(w, k[:, :, j, None]) for j, w in enumerate(liks)]


def edge_weights(r, T):
    """The edge batch over base_weights(r, T, seed=1)."""
    liks = base_weights(r, T, seed=1)
    rng = np.random.default_rng(7000 + T)
    for j, w in enumerate(liks):
        M = w.shape[2]
        down = -rng.integers(0, 601, size=(2, T, M))
        keep = rng.integers(0, M, size=(2, T))
        np.put_along_axis(down, keep[:, :, None], 0, axis=2)
        w[1] = np.ldexp(w[1], down[0])
        w[2, 1::2] = np.ldexp(w[2, 1::2], down[1, 1::2])
        w[3] = np.ldexp(w[3], -1070)
        w[4, 5:13] = np.ldexp(w[4, 5:13], -1070)
        if j == 0:
            w[5] = DBL_MAX
        if j == len(liks) - 1:
            w[6, 5:13] = DBL_MAX
    assert all(np.all(w[3] < np.finfo(np.float64).tiny) and np.all(w[3].max(axis=1) > 0.0) for w in liks)
    return liks


def oracle_args(r, obs, liks):
    """(kinds, cols, liks) over r.tables' columns for soft_util."""
    n = len(r.tables[2])
    Bq, T = (liks[0].shape[:2] if liks else obs.shape[:2])
    kinds, cols, ws = [HARD] * n, [np.full((Bq, T), -1)] * n, [None] * n
    for j, k in enumerate(r.soft):
        kinds[k], cols[k], ws[k] = SOFT, None, liks[j]
    for j, k in enumerate(r.hard):
        cols[k] = obs[:, :, j]
    return kinds, cols, ws


def query_rows(r, rows):
    """The interface rows [B, T, N] as the request's query returns them."""
    if r.digits is None:
        return rows
    return np.concatenate([su.digit_sums(rows, s, c) for s, c in r.digits], axis=2)
