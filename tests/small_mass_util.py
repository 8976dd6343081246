"""Rare-symbol models and observations: inputs whose single steps carry a
tiny evidence mass (tests/test_small_mass_oracle.py, tests/test_gpu_small_mass.py).

Every observed child's table emits code 0 with probability s (0.5 + u) from
every interface state (u uniform in [0, 1), synth.uniform01); its other codes
are ordinary (0.05 + u, normalised to the rest of the row).  A step at which
all ncol observed columns show code 0 then has mass about mu = s^ncol whatever
the state, so the test chooses mu and sets s = mu^(1/ncol).

Declaration order: the children first, then the interface variable, then its
previous-slice copy, as synth.hmm_spec(proper=True) -- the parser
re-normalises each table over its family's lowest-numbered variable, and any
other order would normalise a child's table over the interface and make the
rare column an ordinary one.  Every builder asserts on the compiled tables
(textbook_util.chain_tables, viterbi_util.joint_tables) that column 0 of
every child is at most 2 s.

The reference normalises its messages at every step and adds log m2 - log m1
per step, so its results do not depend on a step's mass until the mass leaves
fp64; the oracles agree with each other down to mu = 1e-150
(tests/test_small_mass_oracle.py), the smallest mass of the matrix.
"""
import functools

import numpy as np

import nip_amd
from nip_amd import synth

import viterbi_util as vu
from textbook_util import chain_tables

MUS = (1e-20, 1e-40, 1e-80, 1e-150)
B = 17
STAR_CARDS = (2, 3, 4, 5)


def col_scale(mu, ncol):
    """s with s^ncol = mu."""
    return float(mu) ** (1.0 / ncol)


def rare_cpt(seed, child_card, parent_configs, s):
    """Textual-order data of `potential (child | parents)`: code 0 has
    probability s (0.5 + u), the other codes share the rest."""
    d = 0.05 + synth.uniform01(seed, child_card * parent_configs).reshape(parent_configs, child_card)
    r = s * (0.5 + synth.uniform01(seed + 7919, parent_configs))
    d[:, 0] = 0.0
    d = d / d.sum(axis=1, keepdims=True) * (1.0 - r)[:, None]
    d[:, 0] = r
    return d.ravel()


class Case:
    """A compiled model with what the tests ask of it: ov / q the observed and
    queried variables, cards the observed cardinalities, tables (A, pi, Es) of
    the interface chain (None where only the port oracle serves), cols(obs) the
    tables' columns of an observation array."""

    def __init__(self, m, ov, q, tables, cols=None, N=None):
        self.m, self.ov, self.q, self.tables = m, ov, q, tables
        self.cards = [m.card(v) for v in ov]
        self.cols = cols or (lambda obs: [obs[:, :, k] for k in range(obs.shape[2])])
        self.N = N if N is not None else (tables[0].shape[0] if tables else None)
        self.ncol = len(ov)


def _assert_rare(Es, s):
    for E in Es:
        assert E[:, 0].max() <= 2 * s, (E[:, 0].max(), s)
        assert E[:, 0].min() >= 0.5 * s * (1 - 1e-12), (E[:, 0].min(), s)


@functools.lru_cache(maxsize=None)
def rare_hmm(N, M=4, s=1e-20, seed=0, proper=True):
    """proper=False declares P0 before P1: the transition is then normalised
    over P0, its rows no longer sum to 1, and the kernels leave their proper
    mode (the ll from per-step masses instead of the final one); the child's
    table stays normalised over the child."""
    nodes = [("M1", M, None), ("P1", N, None), ("P0", N, "P1")]
    if not proper:
        nodes = [nodes[0], nodes[2], nodes[1]]
    pots = [("M1", ["P1"], rare_cpt(700 + N + seed, M, N, s)),
            ("P1", ["P0"], synth.cpt(701 + N + seed, N, N)),
            ("P0", [], synth.cpt(702 + N + seed, N, 1))]
    m = nip_amd.Model.from_spec(nodes, pots)
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    tables = chain_tables(m, P0, P1, [M1])
    _assert_rare(tables[2], s)
    assert proper == bool(np.abs(tables[0].sum(axis=1) - 1.0).max() <= 1e-15)
    return Case(m, [M1], [P1], tables)


@functools.lru_cache(maxsize=None)
def rare_star(N, cards=STAR_CARDS, s=1e-20, observed=(0, 1, 2, 3)):
    """The four-child star of tests/test_gpu_group_columns.py, children first;
    `observed`: the children in the observed list (the others are summed out)."""
    nodes = [("O%d" % k, c, None) for k, c in enumerate(cards)] + [("P1", N, None), ("P0", N, "P1")]
    pots = [("O%d" % k, ["P1"], rare_cpt(710 + N + k, c, N, s)) for k, c in enumerate(cards)]
    pots += [("P1", ["P0"], synth.cpt(720 + N, N, N)), ("P0", [], synth.cpt(721 + N, N, 1))]
    m = nip_amd.Model.from_spec(nodes, pots)
    kids = [m.variable("O%d" % k) for k in range(len(cards))]
    tables = chain_tables(m, m.variable("P0"), m.variable("P1"), kids)
    _assert_rare(tables[2], s)
    observed = tuple(observed)

    def cols(obs):
        return [obs[:, :, observed.index(k)] if k in observed else np.full(obs.shape[:2], -1)
                for k in range(len(cards))]
    return Case(m, [kids[k] for k in observed], [m.variable("P1")], tables, cols)


@functools.lru_cache(maxsize=None)
def rare_demo(N, s=1e-20, a=3, b=4, d=2):
    """Two rare children A1 (a codes), B1 (b) of the interface C0 -> C1 (N
    states) and the hidden parent D1 (d), as test_gpu_post_layout.demo1_mixed."""
    nodes = [("A1", a, None), ("B1", b, None), ("C1", N, None), ("C0", N, "C1"), ("D1", d, None)]
    pots = [("A1", ["C1"], rare_cpt(730 + N, a, N, s)),
            ("B1", ["C1"], rare_cpt(731 + N, b, N, s)),
            ("C0", [], synth.cpt(732 + N, N, 1)),
            ("D1", [], synth.cpt(733 + N, d, 1)),
            ("C1", ["D1", "C0"], synth.cpt(734 + N, N, d * N))]
    m = nip_amd.Model.from_spec(nodes, pots)
    v = {x: m.variable(x) for x in ("A1", "B1", "C0", "C1")}
    tables = chain_tables(m, v["C0"], v["C1"], [v["A1"], v["B1"]])
    _assert_rare(tables[2], s)
    return Case(m, [v["A1"], v["B1"]], [v["C1"]], tables)


@functools.lru_cache(maxsize=None)
def rare_factorial(a=4, b=4, mm=5, s=1e-20):
    """A joint interface {X1, Y1} with one rare child O1 of both."""
    nodes = [("O1", mm, None), ("X1", a, None), ("Y1", b, None), ("X0", a, "X1"), ("Y0", b, "Y1")]
    pots = [("O1", ["X1", "Y1"], rare_cpt(740, mm, a * b, s)),
            ("X1", ["X0"], synth.cpt(741, a, a)),
            ("Y1", ["Y0"], synth.cpt(742, b, b)),
            ("X0", [], synth.cpt(743, a, 1)),
            ("Y0", [], synth.cpt(744, b, 1))]
    m = nip_amd.Model.from_spec(nodes, pots)
    d = m.desc()
    O1 = m.variable("O1")
    A, pi, E = vu.joint_tables(m, d["previous_outgoing"], d["outgoing"], O1)
    _assert_rare([E], s)
    return Case(m, [O1], list(d["outgoing"]), (A, pi, [E]))


@functools.lru_cache(maxsize=None)
def rare_nonleaf(n=5, mm=3, k=3, s=1e-20):
    """synth.nonleaf_spec with a rare code 0 of O1: evidence on O1 and on its
    own child Q1 (the operator chain).  No chain tables: the port oracle is
    the reference."""
    nodes = [("Q1", k, None), ("O1", mm, None), ("P1", n, None), ("P0", n, "P1")]
    pots = [("Q1", ["O1"], synth.cpt(750, k, mm)),
            ("O1", ["P1"], rare_cpt(751, mm, n, s)),
            ("P1", ["P0"], synth.cpt(752, n, n)),
            ("P0", [], synth.cpt(753, n, 1))]
    m = nip_amd.Model.from_spec(nodes, pots)
    E = chain_tables(m, m.variable("P0"), m.variable("P1"), [m.variable("O1")])[2]
    _assert_rare(E, s)
    return Case(m, [m.variable("O1"), m.variable("Q1")], [m.variable("P1")], None, N=n)


def rare_steps(T, B=B, seed=0):
    """(rare [B, T], missing [B, T]) of the per-sequence patterns:
      0      no rare step (the control)
      1      rare at t = 5..12 (across T/2 at T = 24, an 8-step chunk edge, two rescale positions)
      2      rare at t = 0..3
      3      rare at T-5..T-1
      4      every step rare
      5      rare and missing alternating
      6      rare runs of 3 and 4 starting at t = 0 and t = 1 (mod 4)
      7..    random: 25 % rare, 20 % of the other steps missing (t = 0 is
             never missing: a leading missing run puts the reference's BAD_LUCK
             verdict at the mercy of rounding, tests/test_estep_prefix.py)."""
    rng = np.random.default_rng(1000 * T + seed)
    rare = np.zeros((B, T), bool)
    miss = np.zeros((B, T), bool)
    t = np.arange(T)
    if B > 1:
        rare[1, 5:13] = True
    if B > 2:
        rare[2, :4] = True
    if B > 3:
        rare[3, max(0, T - 5):] = True
    if B > 4:
        rare[4] = True
    if B > 5:
        rare[5] = t % 2 == 0
        miss[5] = t % 2 == 1
    if B > 6:
        for start, n in ((0, 3), (5, 4)):
            for k in range(n):
                rare[6, (t % 12) == start + k] = True
    for b in range(7, B):
        u = rng.random(T)
        rare[b] = u < 0.25
        miss[b] = (u >= 0.25) & (u < 0.40)            # 20 % of the other steps
        miss[b, 0] = False
    return rare, miss


def rare_obs(T, cards, B=B, seed=0):
    """int32 [B, T, ncol]: ordinary codes 1 .. card - 1, code 0 in every column
    at a rare step, -1 in every column at a missing one."""
    rng = np.random.default_rng(77 * T + len(cards) + seed)
    obs = np.stack([rng.integers(1, c, size=(B, T)) for c in cards], axis=2).astype(np.int32)
    rare, miss = rare_steps(T, B, seed)
    obs[rare] = 0
    obs[miss] = -1
    return obs
