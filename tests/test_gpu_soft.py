"""Soft (likelihood) evidence on the GPU (nipamd_fb_soft, nipamd_filter_soft,
nip_amd/csrc/soft.hip chain_soft_kernel).

The oracle is soft_util.soft_smoother -- plain numpy over the model's own
tables, pinned to the textbook smoother by tests/test_soft_api.py.  Tolerances
are the project's own (tests/test_gpu_stream.py): rows 1e-12 absolute against
the oracle, ll 1e-11 max(1, |ll|); against the existing GPU entry points rows
2e-12.  Weights are 0.05 + U[0, 1) and hard columns have 20 % missing unless a
test says otherwise.  Batch independence and the host forms are compared bit
for bit.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import nip_amd
from nip_amd import synth

import soft_util as so
import stream_util as su
import viterbi_util as vu
from soft_util import HARD, SOFT
from textbook_util import chain_tables

KERNEL = "chain_soft_kernel"
ROW_TOL, LL_TOL, GPU_TOL = 1e-12, 1e-11, 2e-12
FB, FILTER = "fb", "filter"
DEVICE = {FB: nip_amd.forward_backward_inference_soft, FILTER: nip_amd.forward_inference_soft}
HOSTED = {FB: nip_amd.forward_backward_inference_soft_host, FILTER: nip_amd.forward_inference_soft_host}


def gappy(B, T, cards, seed, frac=0.2):
    rng = np.random.default_rng(seed)
    obs = np.stack([rng.integers(0, c, size=(B, T)) for c in cards], axis=2).astype(np.int32) if cards \
        else np.zeros((B, T, 0), np.int32)
    obs[rng.random(obs.shape) < frac] = -1
    return obs


def weights(B, T, cards, seed):
    """One [B, T, M] array per soft column."""
    rng = np.random.default_rng(seed)
    return [0.05 + rng.random((B, T, c)) for c in cards]


def run(which, m, obs, ov, liks, sv, q, post=None):
    """The device call: obs [B, T, n_obs] int32 (or None), liks the soft
    columns' weight arrays in sv order.  Numpy (rows, ll, status)."""
    o = torch.from_numpy(np.ascontiguousarray(obs, np.int32)).cuda() if obs is not None and len(ov) else None
    w = torch.from_numpy(np.ascontiguousarray(np.concatenate(liks, axis=2))).cuda() if liks else None
    post, ll, st = DEVICE[which](m, o, ov, w, sv, q, post=post)
    assert nip_amd.last_kernel() == KERNEL
    torch.cuda.synchronize()
    return post.cpu().numpy(), ll.cpu().numpy(), st.cpu().numpy()


def check_ll(ll, want):
    err = np.abs(ll - want)
    bound = LL_TOL * np.maximum(1.0, np.abs(want))
    print("max |ll - oracle| %.3g (bound %.3g)" % (err.max(), bound.min()))
    assert np.all(err <= bound), err.max()


def check_rows(rows, want, tol, what="oracle"):
    assert rows.shape == want.shape, (rows.shape, want.shape)
    assert np.isfinite(rows).all()
    err = np.abs(rows - want).max()
    print("max |row - %s| %.3g (bound %.3g)" % (what, err, tol))
    assert err <= tol, err


def oracle_rows(which, tables, kinds, cols, liks):
    A, pi, Es = tables
    smoothed, filtered, ll = so.soft_smoother(A, pi, Es, kinds, cols, liks)
    return (smoothed if which == FB else filtered), ll


# ---------------------------------------------------------------------------
# models, built once

@functools.lru_cache(maxsize=None)
def hmm(N, M, proper, seed=0):
    nodes, pots = synth.hmm_spec(N, M, seed=700 + N + seed, proper=proper)
    m = nip_amd.Model.from_spec(nodes, pots)
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    return m, P1, M1, chain_tables(m, P0, P1, [M1])


@functools.lru_cache(maxsize=None)
def demo1(card):
    nodes, pots = synth.demo1_spec(card, seed=300 + card)
    m = nip_amd.Model.from_spec(nodes, pots)
    v = {s: m.variable(s) for s in ("A1", "B1", "C0", "C1")}
    return m, v, chain_tables(m, v["C0"], v["C1"], [v["A1"], v["B1"]])


@functools.lru_cache(maxsize=None)
def wide():
    nodes, pots = synth.wide_spec(64, 8, seed=77)
    m = nip_amd.Model.from_spec(nodes, pots)
    X0, X1, O1 = m.variable("X0"), m.variable("X1"), m.variable("O1")
    return m, X1, O1, chain_tables(m, X0, X1, [O1])


@functools.lru_cache(maxsize=None)
def five_children():
    nodes = [("P0", 3, "P1"), ("P1", 3, None)] + [("O%d" % k, 2, None) for k in range(5)]
    pots = [("P1", ["P0"], synth.cpt(1, 3, 3)), ("P0", [], synth.cpt(2, 3, 1))]
    pots += [("O%d" % k, ["P1"], synth.cpt(3 + k, 2, 3)) for k in range(5)]
    m = nip_amd.Model.from_spec(nodes, pots)
    ov = [m.variable("O%d" % k) for k in range(5)]
    return m, m.variable("P1"), ov, chain_tables(m, m.variable("P0"), m.variable("P1"), ov)


@functools.lru_cache(maxsize=None)
def factorial():
    nodes, pots = synth.factorial_spec(4, 4, 5, seed=61)
    m = nip_amd.Model.from_spec(nodes, pots)
    d = m.desc()
    cur, prev = d["outgoing"], d["previous_outgoing"]
    O1 = m.variable("O1")
    A, pi, E = vu.joint_tables(m, prev, cur, O1)
    return m, cur, O1, (A, pi, [E])


# ---------------------------------------------------------------------------
# 1. against the oracle

@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("T", [1, 2, 65])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("proper", [False, True])
@pytest.mark.parametrize("N,M", [(3, 4), (16, 16)])
def test_hmm_soft_child(N, M, proper, B, T, which):
    m, P1, M1, tables = hmm(N, M, proper)
    liks = weights(B, T, (M,), 13 * B + T + N)
    rows, ll, st = run(which, m, None, [], liks, [M1], [P1])
    want, want_ll = oracle_rows(which, tables, [SOFT], [None], liks)
    check_rows(rows, want, ROW_TOL)
    check_ll(ll, want_ll)
    assert np.all(st == 0)


@pytest.mark.parametrize("which", [FB, FILTER])
def test_weight_vector_longer_than_the_group(which):
    """A 3-state parent (NP = 16) with a 20-state child: the weight-load loop."""
    m, P1, M1, tables = hmm(3, 20, False)
    B, T = 5, 33
    liks = weights(B, T, (20,), 5)
    rows, ll, st = run(which, m, None, [], liks, [M1], [P1])
    want, want_ll = oracle_rows(which, tables, [SOFT], [None], liks)
    check_rows(rows, want, ROW_TOL)
    check_ll(ll, want_ll)
    assert np.all(st == 0)


@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("mix", ["a-soft-b-hard", "both-soft", "a-hard-b-unlisted"])
@pytest.mark.parametrize("card", [17, 20, 32, 33])
def test_demo1(card, mix, which):
    """card <= 32: NP = 32, two sequences per wave, B = 3 leaves the last wave
    half full; card 33: NP = 64."""
    m, v, tables = demo1(card)
    B, T = (3 if card <= 32 else 2), 33
    obs = gappy(B, T, (card,), 7 + card)
    wa, wb = weights(B, T, (card, card), 9 + card)
    none = np.full((B, T), -1)
    if mix == "a-soft-b-hard":
        got = run(which, m, obs, [v["B1"]], [wa], [v["A1"]], [v["C1"]])
        want, want_ll = oracle_rows(which, tables, [SOFT, HARD], [None, obs[:, :, 0]], [wa, None])
    elif mix == "both-soft":
        got = run(which, m, None, [], [wa, wb], [v["A1"], v["B1"]], [v["C1"]])
        want, want_ll = oracle_rows(which, tables, [SOFT, SOFT], [None, None], [wa, wb])
    else:
        got = run(which, m, obs, [v["A1"]], [], [], [v["C1"]])
        want, want_ll = oracle_rows(which, tables, [HARD, HARD], [obs[:, :, 0], none], [None, None])
    check_rows(got[0], want, ROW_TOL)
    check_ll(got[1], want_ll)
    assert np.all(got[2] == 0)


@pytest.mark.parametrize("which", [FB, FILTER])
def test_wide64(which):
    m, X1, O1, tables = wide()
    B, T = 2, 9
    liks = weights(B, T, (8,), 64)
    rows, ll, st = run(which, m, None, [], liks, [O1], [X1])
    want, want_ll = oracle_rows(which, tables, [SOFT], [None], liks)
    check_rows(rows, want, ROW_TOL)
    check_ll(ll, want_ll)
    assert np.all(st == 0)


@pytest.mark.parametrize("which", [FB, FILTER])
def test_four_soft_columns(which):
    m, P1, ov, tables = five_children()
    B, T = 6, 5
    liks = weights(B, T, (2, 2, 2, 2), 45)
    rows, ll, st = run(which, m, None, [], liks, ov[:4], [P1])
    want, want_ll = oracle_rows(which, tables, [SOFT] * 4 + [HARD], [None] * 4 + [np.full((B, T), -1)], liks + [None])
    check_rows(rows, want, ROW_TOL)
    check_ll(ll, want_ll)
    assert np.all(st == 0)


@pytest.mark.parametrize("which", [FB, FILTER])
def test_joint_interface(which):
    m, cur, O1, tables = factorial()
    X1, Y1 = m.variable("X1"), m.variable("Y1")
    stride = {cur[0]: 1, cur[1]: m.card(cur[0])}
    B, T = 5, 30
    liks = weights(B, T, (5,), 61)
    joint, want_ll = oracle_rows(which, tables, [SOFT], [None], liks)
    wx, wy = su.digit_sums(joint, stride[X1], 4), su.digit_sums(joint, stride[Y1], 4)
    xy, ll, st = run(which, m, None, [], liks, [O1], [X1, Y1])
    check_rows(xy, np.concatenate([wx, wy], axis=2), ROW_TOL)
    check_ll(ll, want_ll)
    assert np.all(st == 0)
    yx, ll2, _ = run(which, m, None, [], liks, [O1], [Y1, X1])
    check_rows(yx, np.concatenate([wy, wx], axis=2), ROW_TOL)
    check_ll(ll2, want_ll)
    y, ll3, _ = run(which, m, None, [], liks, [O1], [Y1])
    check_rows(y, wy, ROW_TOL)
    check_ll(ll3, want_ll)


@pytest.mark.parametrize("which", [FB, FILTER])
def test_soft_evidence_on_the_interface_variable(which):
    m, P1, M1, (A, pi, Es) = hmm(3, 4, False)
    B, T = 5, 20
    liks = weights(B, T, (3,), 33)
    rows, ll, st = run(which, m, None, [], liks, [P1], [P1])
    want, want_ll = oracle_rows(which, (A, pi, Es + [np.eye(3)]), [HARD, SOFT], [np.full((B, T), -1), None],
                                [None] + liks)
    check_rows(rows, want, ROW_TOL)
    check_ll(ll, want_ll)
    assert np.all(st == 0)


# ---------------------------------------------------------------------------
# 2. against the existing entry points

EXISTING = {FB: nip_amd.forward_backward_inference, FILTER: nip_amd.forward_inference}


def _parity_case(name):
    if name == "hmm16":
        m, P1, M1, _ = hmm(16, 16, False)
        return m, [M1], [P1], (16,)
    m, v, _ = demo1(20)
    return m, [v["A1"], v["B1"]], [v["C1"]], (20, 20)


@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("form", ["no-soft-columns", "one-hot-weights"])
@pytest.mark.parametrize("name", ["hmm16", "demo1-20"])
def test_parity_with_hard_evidence(name, form, which):
    m, ov, q, cards = _parity_case(name)
    B, T = 5, 40
    obs = gappy(B, T, cards, 21 + len(name))
    post, ll, st = EXISTING[which](m, torch.from_numpy(obs).cuda(), ov, q)
    torch.cuda.synchronize()
    if form == "no-soft-columns":
        got = run(which, m, obs, ov, [], [], q)
    else:
        liks = []
        for k, c in enumerate(cards):
            w = np.eye(c)[np.maximum(obs[:, :, k], 0)]
            w[obs[:, :, k] < 0] = 1.0
            liks.append(w)
        got = run(which, m, None, [], liks, ov, q)
    check_rows(got[0], post.cpu().numpy(), GPU_TOL, "the hard entry point")
    check_ll(got[1], ll.cpu().numpy())
    assert np.array_equal(got[2], st.cpu().numpy())


@pytest.mark.parametrize("which", [FB, FILTER])
def test_posterior_rows_fed_back_as_evidence(which):
    """The rows nipamd_fb writes for [P1] are the likelihood rows of
    soft_vars = [P1] of a second model, unchanged."""
    m, P1, M1, _ = hmm(16, 16, False)
    m2, Q1, _, (A, pi, Es) = hmm(16, 16, True, seed=5)
    B, T = 5, 40
    obs = gappy(B, T, (16,), 91)
    post, _, _ = nip_amd.forward_backward_inference(m, torch.from_numpy(obs).cuda(), [M1], [P1])
    rows, ll, st = DEVICE[which](m2, None, [], post, [Q1], [Q1])
    assert nip_amd.last_kernel() == KERNEL
    torch.cuda.synchronize()
    fed = post.cpu().numpy()
    want, want_ll = oracle_rows(which, (A, pi, Es + [np.eye(16)]), [HARD, SOFT], [np.full((B, T), -1), None],
                                [None, fed])
    check_rows(rows.cpu().numpy(), want, ROW_TOL)
    check_ll(ll.cpu().numpy(), want_ll)
    assert np.all(st.cpu().numpy() == 0)


# ---------------------------------------------------------------------------
# 3. dead sequences and bad weights

def _dead_case():
    m, P1, M1, tables = hmm(3, 4, False)
    return m, P1, M1, tables, weights(4, 10, (4,), 17)[0]


@pytest.mark.parametrize("which", [FB, FILTER])
def test_a_sequence_without_mass(which):
    m, P1, M1, tables, w = _dead_case()
    good = run(which, m, None, [], [w], [M1], [P1])
    bad = w.copy()
    bad[1, 6] = 0.0
    rows, ll, st = run(which, m, None, [], [bad], [M1], [P1])
    assert list(st) == [0, 1, 0, 0] and ll[1] == -vu.DBL_MAX
    if which == FB:
        assert np.all(rows[1] == 0.0)
    else:
        want, _ = oracle_rows(which, tables, [SOFT], [None], [bad])
        check_rows(rows[1, :6], want[1, :6], ROW_TOL)
        assert np.all(rows[1, 6:] == 0.0)
    for k in (0, 2, 3):
        assert np.array_equal(rows[k], good[0][k]) and ll[k] == good[1][k]


@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("value", [np.nan, -1.0, np.inf])
def test_a_bad_weight(value, which):
    m, P1, M1, tables, w = _dead_case()
    good = run(which, m, None, [], [w], [M1], [P1])
    bad = w.copy()
    bad[2, 3, 1] = value
    rows, ll, st = run(which, m, None, [], [bad], [M1], [P1])
    assert list(st) == [0, 0, nip_amd.STATUS_BAD_EVIDENCE | nip_amd.STATUS_ZERO_MASS, 0]
    assert ll[2] == -vu.DBL_MAX
    assert not np.isnan(rows).any() and not np.isnan(ll).any()
    if which == FB:
        assert np.all(rows[2] == 0.0)
    else:
        assert np.array_equal(rows[2, :3], good[0][2, :3])
        assert np.all(rows[2, 3:] == 0.0)
    for k in (0, 1, 3):
        assert np.array_equal(rows[k], good[0][k]) and ll[k] == good[1][k]


# ---------------------------------------------------------------------------
# 4. a sequence's results are its own, bit for bit

@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("name", ["hmm16", "demo1-33"])
def test_batch_independence(name, which):
    B, T = 7, 20
    if name == "hmm16":
        m, P1, M1, _ = hmm(16, 16, False)
        ov, sv, q, obs, liks = [], [M1], [P1], None, weights(B, T, (16,), 3)
    else:
        m, v, _ = demo1(33)
        ov, sv, q = [v["B1"]], [v["A1"]], [v["C1"]]
        obs, liks = gappy(B, T, (33,), 4), weights(B, T, (33,), 5)
    cut = lambda b: (None if obs is None else obs[b], [w[b] for w in liks])
    whole = run(which, m, obs, ov, liks, sv, q)
    o, w = cut(slice(None, None, -1))
    rev = run(which, m, o, ov, w, sv, q)
    for a, b in zip(whole, rev):
        assert np.array_equal(a, b[::-1])
    for k in range(B):
        o, w = cut(slice(k, k + 1))
        alone = run(which, m, o, ov, w, sv, q)
        for a, b in zip(whole, alone):
            assert np.array_equal(a[k:k + 1], b), k


# ---------------------------------------------------------------------------
# 5. states the forward pass never reaches

@functools.lru_cache(maxsize=None)
def two_blocks():
    """A 4-state chain of two 2-state blocks that never mix; the prior is on
    the first block, and the second block's emissions are the ones the evidence
    of test_unreachable_block favours: beta on the first block shrinks against
    the second by a factor of about 0.7 per step (0.8 x 0.55 + 0.2 x 1.0 against
    0.2 x 0.55 + 0.8 x 1.0 in the mean), 1e-170 over 1100 steps -- as steep as
    fp64 lets the oracle itself go, which normalises beta by its sum at every
    step and loses the first block below 1e-308."""
    A = np.array([[0.7, 0.3, 0.0, 0.0], [0.4, 0.6, 0.0, 0.0], [0.0, 0.0, 0.5, 0.5], [0.0, 0.0, 0.2, 0.8]])
    E = np.array([[0.45, 0.35, 0.1, 0.1], [0.35, 0.45, 0.1, 0.1], [0.1, 0.1, 0.45, 0.35], [0.1, 0.1, 0.35, 0.45]])
    pi = np.array([0.5, 0.5, 0.0, 0.0])
    nodes = [("M1", 4, None), ("P1", 4, None), ("P0", 4, "P1")]
    pots = [("M1", ["P1"], E.ravel()), ("P1", ["P0"], A.ravel()), ("P0", [], pi)]
    m = nip_amd.Model.from_spec(nodes, pots)
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    tables = chain_tables(m, P0, P1, [M1])
    assert np.all(tables[0][:2, 2:] == 0.0) and np.all(tables[0][2:, :2] == 0.0) and np.all(tables[1][2:] == 0.0)
    return m, P1, M1, tables


def test_unreachable_block():
    m, P1, M1, tables = two_blocks()
    B, T = 2, 1100
    rng = np.random.default_rng(12)
    w = 0.05 + rng.random((B, T, 4))
    w[:, :, 2:] += 0.45                                     # the second block's symbols
    rows, ll, st = run(FB, m, None, [], [w], [M1], [P1])
    want, want_ll = oracle_rows(FB, tables, [SOFT], [None], [w])
    check_rows(rows, want, ROW_TOL)
    check_ll(ll, want_ll)
    assert np.all(st == 0) and np.all(rows[:, :, 2:] == 0.0)


# ---------------------------------------------------------------------------
# 6. the host forms, and the rows' bounds

@pytest.mark.parametrize("which", [FB, FILTER])
def test_host_form_is_the_device_form(which):
    m, P1, M1, _ = hmm(16, 16, False)
    B, T = 3, 7
    obs = gappy(B, T, (16,), 2)
    liks = weights(B, T, (16,), 8)
    want = run(which, m, obs, [M1], liks, [P1], [P1])
    post, ll, st = HOSTED[which](m, obs, [M1], liks[0], [P1], [P1])
    assert np.array_equal(post, want[0]) and np.array_equal(ll, want[1])
    assert np.array_equal(st.astype(np.int32), want[2])
    want = run(which, m, None, [], liks, [M1], [P1])
    post, ll, st = HOSTED[which](m, None, [], liks[0], [M1], [P1])
    assert np.array_equal(post, want[0]) and np.array_equal(ll, want[1])


@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("name", ["demo1-20", "factorial"])
def test_guard_bands(name, which):
    """post is a slice of a larger tensor with 64 doubles of sentinel on either side."""
    B, T = 3, 11
    if name == "demo1-20":
        m, v, _ = demo1(20)
        sv, q, cards, width = [v["A1"]], [v["C1"]], (20,), 20
    else:
        m, cur, O1, _ = factorial()
        sv, q, cards, width = [O1], [m.variable("Y1")], (5,), 4
    liks = weights(B, T, cards, 19)
    n = B * T * width
    big = torch.full((n + 128,), -7.25, dtype=torch.float64, device="cuda")
    post = big[64:64 + n].view(B, T, width)
    rows, _, st = run(which, m, None, [], liks, sv, q, post=post)
    big = big.cpu().numpy()
    assert np.all(big[:64] == -7.25) and np.all(big[64 + n:] == -7.25)
    assert np.all(st == 0) and np.all(rows >= 0.0) and np.abs(rows.sum(axis=2) - 1.0).max() <= 1e-12


def test_python_argument_checks():
    m, P1, M1, _ = hmm(3, 4, False)
    w = torch.ones((2, 3, 4), dtype=torch.float64, device="cuda")
    for bad in (w.float(), w[:, :, :3].contiguous(), w.cpu(), w.transpose(0, 1), None):
        with pytest.raises(nip_amd.NipError) as e:
            nip_amd.forward_backward_inference_soft(m, None, [], bad, [M1], [P1])
        assert e.value.code == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    with pytest.raises(nip_amd.NipError) as e:
        nip_amd.forward_inference_soft(m, None, [], w, [M1], [P1], post=torch.zeros((2, 3, 3), device="cuda"))
    assert e.value.code == nip_amd.NIP_ERROR_INVALID_ARGUMENT
