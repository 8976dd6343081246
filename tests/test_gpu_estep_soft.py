"""The e_step under soft evidence on the GPU (nipamd_estep_soft_partial,
nipamd_estep_soft, nip_amd/csrc/estep_soft.hip chain_estep_soft_kernel) and
em_learn_soft.

The oracle is estep_soft_util.soft_sums -- plain numpy over the model's own
tables, pinned to textbook_util.hmm_estep_torch by
tests/test_estep_soft_api.py.  Tolerances are the project's own: counts and
slab sums 1e-11 max(1, |count|) (tests/test_gpu_estep_wide.py), ll 1e-11
max(1, |ll|) (tests/test_gpu_soft.py check_ll), em_learn curves 1e-10
(tests/test_gpu_train.py).  Weights are 0.05 + U[0, 1) unless a test says
otherwise.  Scaling, batch independence, the tree and the host form are
compared bit for bit.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import nip_amd
from nip_amd import synth
from nip_amd.em import tree_sum

import estep_soft_util as es
import test_gpu_soft as tg
from em_util import close
from soft_util import HARD, SOFT
from textbook_util import chain_tables
from viterbi_util import DBL_MAX, LN2

KERNEL = "chain_estep_soft_kernel"
CNT_RTOL, CURVE_RTOL = 1e-11, 1e-10
EPS = np.finfo(np.float64).eps
UNSUPPORTED, INVALID = nip_amd.NIPAMD_ERROR_UNSUPPORTED, nip_amd.NIP_ERROR_INVALID_ARGUMENT


def dev(obs, ov, liks):
    o = torch.from_numpy(np.ascontiguousarray(obs, np.int32)).cuda() if obs is not None and len(ov) else None
    w = torch.from_numpy(np.ascontiguousarray(np.concatenate(liks, axis=2))).cuda() if liks else None
    return o, w


def run_partial(m, obs, ov, liks, sv, **bufs):
    """The device call on numpy inputs (liks: the soft columns' weight arrays
    in sv order).  Numpy (partial, ll, status)."""
    o, w = dev(obs, ov, liks)
    p, ll, st = nip_amd.estep_partial_soft(m, o, ov, w, sv, **bufs)
    assert nip_amd.last_kernel() == KERNEL
    torch.cuda.synchronize()
    return p.cpu().numpy(), ll.cpu().numpy(), st.cpu().numpy()


def run_counts(m, obs, ov, liks, sv, **bufs):
    o, w = dev(obs, ov, liks)
    c, ll, st = nip_amd.e_step_soft(m, o, ov, w, sv, **bufs)
    assert nip_amd.last_kernel() == KERNEL
    torch.cuda.synchronize()
    return c.cpu().numpy(), ll.cpu().numpy(), st.cpu().numpy()


def check_close(got, want, what):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print("max |%s - oracle| / max(1, |oracle|) %.3g (bound %.3g)" % (what, err.max(), CNT_RTOL))
    assert close(got, want, CNT_RTOL), err.max()


def check_slab(partial, N, sums):
    """The partial against the oracle's sums: the slab, zeros up to the tag, the tag (0, 0, 1)."""
    want = es.slab(N, *sums[:3])
    check_close(partial[:want.size], want, "slab")
    assert np.all(partial[want.size:-3] == 0.0) and partial[-3:].tolist() == [0.0, 0.0, 1.0]


@functools.lru_cache(maxsize=None)
def star(N, cards, seed=40):
    """An N-state chain with one leaf child per entry of cards.  Returns (model,
    P0, P1, the children, (A, pi, Es))."""
    nodes = [("P0", N, "P1"), ("P1", N, None)] + [("O%d" % k, c, None) for k, c in enumerate(cards)]
    pots = [("P1", ["P0"], synth.cpt(seed, N, N)), ("P0", [], synth.cpt(seed + 1, N, 1))]
    pots += [("O%d" % k, ["P1"], synth.cpt(seed + 2 + k, c, N)) for k, c in enumerate(cards)]
    m = nip_amd.Model.from_spec(nodes, pots)
    P0, P1 = m.variable("P0"), m.variable("P1")
    kids = [m.variable("O%d" % k) for k in range(len(cards))]
    return m, P0, P1, kids, chain_tables(m, P0, P1, kids)


def hmm_star(N, M, proper):
    m, P1, M1, tables = tg.hmm(N, M, proper)
    return m, m.variable("P0"), P1, M1, tables


# ---------------------------------------------------------------------------
# 1. against the oracle

@pytest.mark.parametrize("T", [1, 2, 65])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("proper", [False, True])
@pytest.mark.parametrize("N,M", [(3, 4), (16, 16)])
def test_hmm_soft_child(N, M, proper, B, T):
    m, P0, P1, M1, (A, pi, Es) = hmm_star(N, M, proper)
    liks = tg.weights(B, T, (M,), 13 * B + T + N)
    sums = es.soft_sums(A, pi, Es, [SOFT], [None], liks)
    partial, ll, st = run_partial(m, None, [], liks, [M1])
    check_slab(partial, N, sums)
    tg.check_ll(ll, sums[3])
    assert np.all(st == 0)
    cnt, ll2, st2 = run_counts(m, None, [], liks, [M1])
    check_close(cnt, es.star_counts(m, P0, P1, [M1], A, Es, *sums[:3]), "counts")
    assert np.array_equal(ll2, ll) and np.array_equal(st2, st)


# ---------------------------------------------------------------------------
# 2. the other group widths and paths

def test_np32():
    """20 states: NP = 32, two sequences per wave, B = 3 leaves the last wave half full."""
    m, P0, P1, M1, (A, pi, Es) = hmm_star(20, 16, False)
    B, T = 3, 33
    liks = tg.weights(B, T, (16,), 32)
    sums = es.soft_sums(A, pi, Es, [SOFT], [None], liks)
    partial, ll, st = run_partial(m, None, [], liks, [M1])
    check_slab(partial, 20, sums)
    tg.check_ll(ll, sums[3])
    assert np.all(st == 0)
    cnt, _, _ = run_counts(m, None, [], liks, [M1])
    check_close(cnt, es.star_counts(m, P0, P1, [M1], A, Es, *sums[:3]), "counts")


def test_np64_hidden_parents():
    """synth.wide_spec(64, 8): NP = 64, the transition folded over two hidden parents."""
    m, X1, O1, (A, pi, Es) = tg.wide()
    B, T = 3, 33
    liks = tg.weights(B, T, (8,), 64)
    sums = es.soft_sums(A, pi, Es, [SOFT], [None], liks)
    partial, ll, st = run_partial(m, None, [], liks, [O1])
    check_slab(partial, 64, sums)
    tg.check_ll(ll, sums[3])
    assert np.all(st == 0)


def test_weight_vector_longer_than_the_group():
    """A 3-state parent (NP = 16) with a 40-state child: the vector's later pieces."""
    m, P0, P1, M1, (A, pi, Es) = hmm_star(3, 40, False)
    B, T = 5, 33
    liks = tg.weights(B, T, (40,), 5)
    sums = es.soft_sums(A, pi, Es, [SOFT], [None], liks)
    partial, ll, st = run_partial(m, None, [], liks, [M1])
    check_slab(partial, 3, sums)
    tg.check_ll(ll, sums[3])
    assert np.all(st == 0)
    cnt, _, _ = run_counts(m, None, [], liks, [M1])
    check_close(cnt, es.star_counts(m, P0, P1, [M1], A, Es, *sums[:3]), "counts")


def test_three_children_hard_soft_and_unnamed():
    """A star of three children: the first hard (with -1, and one out-of-range
    code, whose sequence is dead), the second soft, the third named by no column."""
    m, P0, P1, kids, (A, pi, Es) = star(5, (3, 4, 2))
    B, T = 6, 17
    obs = tg.gappy(B, T, (3,), 71)
    obs[0, :3] = -1
    obs[4, 9, 0] = 3                                        # out of range
    liks = tg.weights(B, T, (4,), 72)
    none = np.full((B, T), -1)
    sums = es.soft_sums(A, pi, Es, [HARD, SOFT, HARD], [obs[:, :, 0], None, none], [None, liks[0], None])
    cnt, ll, st = run_counts(m, obs, [kids[0]], liks, [kids[1]])
    assert list(st) == [0, 0, 0, 0, 3, 0] and ll[4] == -DBL_MAX
    assert np.array_equal(st, sums[4])
    check_close(cnt, es.star_counts(m, P0, P1, kids, A, Es, *sums[:3]), "counts")
    live = st == 0
    tg.check_ll(ll[live], sums[3][live])


def test_four_soft_columns():
    """Four soft columns, listed in another order than the plan's children."""
    m, P0, P1, kids, (A, pi, Es) = star(5, (3, 4, 2, 6))
    B, T = 6, 9
    order = [3, 1, 0, 2]
    liks = tg.weights(B, T, tuple((3, 4, 2, 6)[k] for k in order), 45)
    by_child = [liks[order.index(k)] for k in range(4)]
    sums = es.soft_sums(A, pi, Es, [SOFT] * 4, [None] * 4, by_child)
    cnt, ll, st = run_counts(m, None, [], liks, [kids[k] for k in order])
    check_close(cnt, es.star_counts(m, P0, P1, kids, A, Es, *sums[:3]), "counts")
    tg.check_ll(ll, sums[3])
    assert np.all(st == 0)


# ---------------------------------------------------------------------------
# 3. parity with the hard e_step

def _parity_case(name):
    if name == "hmm16":
        m, P1, M1, _ = tg.hmm(16, 16, False)
        return m, [M1], (16,)
    if name == "demo1-20":
        m, v, _ = tg.demo1(20)
        return m, [v["A1"], v["B1"]], (20, 20)
    m, X1, O1, _ = tg.wide()
    return m, [O1], (8,)


@pytest.mark.parametrize("form", ["all-soft", "hard-columns-only", "first-soft-rest-hard"])
@pytest.mark.parametrize("name", ["hmm16", "demo1-20", "wide64"])
def test_parity_with_the_hard_e_step(name, form):
    """One-hot weights are the codes and all-ones weights the code -1: the
    counts, the ll and the status of e_step on the codes.  Step 0 is observed,
    so that e_step's verdict on a leading missing run stays out of it."""
    m, ov, cards = _parity_case(name)
    B, T = 5, 40
    obs = tg.gappy(B, T, cards, 21 + len(name))
    obs[:, 0] = tg.gappy(B, 1, cards, 5, frac=0.0)[:, 0]
    want, want_ll, want_st = nip_amd.e_step(m, torch.from_numpy(obs).cuda(), ov)
    assert nip_amd.last_kernel() != KERNEL
    torch.cuda.synchronize()
    assert np.all(want_st.cpu().numpy() == 0)
    hot = [es.one_hot(obs[:, :, k], c) for k, c in enumerate(cards)]
    if form == "all-soft":
        got = run_counts(m, None, [], hot, ov)
    elif form == "hard-columns-only":
        got = run_counts(m, obs, ov, [], [])
    else:
        got = run_counts(m, obs[:, :, 1:], ov[1:], hot[:1], ov[:1])
    check_close(got[0], want.cpu().numpy(), "counts")
    tg.check_ll(got[1], want_ll.cpu().numpy())
    assert np.all(got[2] == 0)


# ---------------------------------------------------------------------------
# 4. the weights' scale

def _scale_case(name):
    if name == "hmm16":
        m, P0, P1, M1, tables = hmm_star(16, 16, False)
        return m, P0, P1, [M1], tables, (16,)
    m, P0, P1, kids, tables = star(5, (3, 4))
    return m, P0, P1, kids, tables, (3, 4)


@pytest.mark.parametrize("name", ["hmm16", "star-two-soft"])
def test_powers_of_two_change_no_bit_of_the_partial(name):
    m, P0, P1, kids, tables, cards = _scale_case(name)
    B, T = 5, 24
    liks = tg.weights(B, T, cards, 8)
    rng = np.random.default_rng(9)
    js = [rng.integers(-900, 901, size=(B, T)) for _ in cards]
    scaled = [np.ldexp(w, j[:, :, None]) for w, j in zip(liks, js)]
    assert all(np.isfinite(w).all() and np.all(w >= np.finfo(np.float64).tiny) for w in scaled)
    p0, ll0, st0 = run_partial(m, None, [], liks, kids)
    p1, ll1, st1 = run_partial(m, None, [], scaled, kids)
    assert np.array_equal(p0, p1)
    assert np.all(st0 == 0) and np.all(st1 == 0)
    K = sum(j.sum(axis=1) for j in js)
    err = np.abs(ll1 - K * LN2 - ll0)
    bound = 1e-11 * np.maximum(1.0, np.abs(ll0)) + 4 * EPS * np.abs(ll1)
    print("|ll - K ln 2 - ll_0| %s" % " ".join("%.2g" % e for e in err))
    assert np.all(err <= bound), (err.tolist(), bound.tolist())


@pytest.mark.parametrize("name", ["hmm16", "star-two-soft"])
def test_denormal_and_largest_weights(name):
    """One all-denormal vector and one vector whose largest weight is DBL_MAX."""
    m, P0, P1, kids, (A, pi, Es), cards = _scale_case(name)
    B, T = 4, 12
    liks = tg.weights(B, T, cards, 18)
    liks[0][1, 5] = np.ldexp(liks[0][1, 5], -1070)
    liks[-1][2, 7] = liks[-1][2, 7] / liks[-1][2, 7].max() * DBL_MAX
    assert liks[0][1, 5].max() < np.finfo(np.float64).tiny and liks[-1][2, 7].max() == DBL_MAX
    sums = es.soft_sums(A, pi, Es, [SOFT] * len(cards), [None] * len(cards), liks)
    cnt, ll, st = run_counts(m, None, [], liks, kids)
    assert np.all(st == 0) and np.all(sums[4] == 0)
    check_close(cnt, es.star_counts(m, P0, P1, kids, A, Es, *sums[:3]), "counts")
    tg.check_ll(ll, sums[3])


# ---------------------------------------------------------------------------
# 5. dead sequences and bad weights

def _dead_case():
    m, P0, P1, M1, tables = hmm_star(3, 4, False)
    return m, M1, tg.weights(4, 10, (4,), 17)[0]


def test_an_all_zero_vector():
    m, M1, w = _dead_case()
    good = run_partial(m, None, [], [w], [M1])
    bad = w.copy()
    bad[1, 3] = 0.0
    p, ll, st = run_partial(m, None, [], [bad], [M1])
    assert list(st) == [0, 3, 0, 0] and ll[1] == -DBL_MAX
    assert np.isfinite(p).all()
    for k in (0, 2, 3):
        assert ll[k] == good[1][k]
    others = run_partial(m, None, [], [w[[0, 2, 3]]], [M1])
    check_close(p, others[0], "partial")


@pytest.mark.parametrize("value", [np.nan, -1.0, np.inf])
def test_a_bad_weight(value):
    m, M1, w = _dead_case()
    bad = w.copy()
    bad[2, 3, 1] = value
    p, ll, st = run_partial(m, None, [], [bad], [M1])
    assert list(st) == [0, 0, 7, 0] and ll[2] == -DBL_MAX
    assert np.isfinite(p).all() and not np.isnan(ll).any()
    others = run_partial(m, None, [], [w[[0, 1, 3]]], [M1])
    check_close(p, others[0], "partial")


@pytest.mark.parametrize("value", [0.0, np.nan])
def test_a_dead_sequence_adds_nothing(value):
    """[live, dead] and [live] alone: the same partial, bit for bit."""
    m, M1, w = _dead_case()
    two = w[:2].copy()
    two[1, 3] = value
    p2, ll2, st2 = run_partial(m, None, [], [two], [M1])
    p1, ll1, st1 = run_partial(m, None, [], [w[:1]], [M1])
    assert st2[0] == 0 and st2[1] != 0 and st1[0] == 0
    assert np.array_equal(p2, p1) and ll2[0] == ll1[0]


# ---------------------------------------------------------------------------
# 6. the tree, the two halves and the host form

def test_tree_of_shards():
    m, P0, P1, M1, _ = hmm_star(16, 16, False)
    B, T = 8, 20
    obs = tg.gappy(B, T, (16,), 3)
    m2, v, _ = tg.demo1(20)
    for mm, ov, sv, o, liks in ((m, [], [M1], None, tg.weights(B, T, (16,), 3)),
                                (m2, [v["B1"]], [v["A1"]], tg.gappy(B, T, (20,), 4), tg.weights(B, T, (20,), 5))):
        whole = torch.from_numpy(run_partial(mm, o, ov, liks, sv)[0])
        halves = [torch.from_numpy(run_partial(mm, None if o is None else o[h], ov, [w[h] for w in liks], sv)[0])
                  for h in (slice(0, 4), slice(4, 8))]
        comb = tree_sum(torch.stack(halves))
        assert torch.equal(comb[:-3], whole[:-3])
        assert comb[-3:].tolist() == [0.0, 0.0, 2.0] and whole[-3:].tolist() == [0.0, 0.0, 1.0]


def test_batch_independence():
    """A sequence's slab is its own: the partial of one sequence, whatever batch it sits in."""
    m, P0, P1, M1, _ = hmm_star(16, 16, False)
    B, T = 7, 20
    liks = tg.weights(B, T, (16,), 3)
    _, ll, _ = run_partial(m, None, [], liks, [M1])
    rev_p, rev_ll, _ = run_partial(m, None, [], [liks[0][::-1]], [M1])
    assert np.array_equal(ll, rev_ll[::-1])
    for k in (0, 3, 6):
        alone = run_partial(m, None, [], [liks[0][k:k + 1]], [M1])
        pair = liks[0][[k, k]].copy()
        pair[1, 2] = 0.0                                    # a dead neighbour in the same wave
        assert np.array_equal(run_partial(m, None, [], [pair], [M1])[0], alone[0])
        assert alone[1][0] == ll[k]


def test_partial_and_finalize_are_the_e_step():
    m, v, _ = tg.demo1(20)
    B, T = 5, 20
    obs, liks = tg.gappy(B, T, (20,), 4), tg.weights(B, T, (20,), 5)
    o, w = dev(obs, [v["B1"]], liks)
    p, ll, st = nip_amd.estep_partial_soft(m, o, [v["B1"]], w, [v["A1"]])
    two = nip_amd.estep_finalize(m, p, None)
    one, ll1, st1 = nip_amd.e_step_soft(m, o, [v["B1"]], w, [v["A1"]])
    assert torch.equal(one, two) and torch.equal(ll, ll1) and torch.equal(st, st1)


def test_host_form_is_the_device_form():
    m, P0, P1, M1, _ = hmm_star(16, 16, False)
    B, T = 3, 7
    liks = tg.weights(B, T, (16,), 8)
    want = run_counts(m, None, [], liks, [M1])
    cnt, ll, st = nip_amd.e_step_soft_host(m, None, [], liks[0], [M1])
    assert np.array_equal(cnt, want[0]) and np.array_equal(ll, want[1])
    assert np.array_equal(st.astype(np.int32), want[2])
    m2, v, _ = tg.demo1(20)
    obs, liks = tg.gappy(B, T, (20,), 2), tg.weights(B, T, (20,), 8)
    want = run_counts(m2, obs, [v["B1"]], liks, [v["A1"]])
    cnt, ll, st = nip_amd.e_step_soft_host(m2, obs, [v["B1"]], liks[0], [v["A1"]])
    assert np.array_equal(cnt, want[0]) and np.array_equal(ll, want[1])
    assert np.array_equal(st.astype(np.int32), want[2])


# ---------------------------------------------------------------------------
# 7. the outputs' bounds

def banded(n, dtype, value):
    big = torch.full((n + 128,), value, dtype=dtype, device="cuda")
    return big, big[64:64 + n]


def intact(big, n, value):
    b = big.cpu().numpy()
    return np.all(b[:64] == value) and np.all(b[64 + n:] == value)


@pytest.mark.parametrize("name", ["hmm3", "demo1-20", "wide64"])
def test_guard_bands(name):
    """partial, counts, ll and status are slices of larger tensors with 64 elements of sentinel on either side."""
    B, T = 3, 11
    if name == "hmm3":
        m, P0, P1, M1, _ = hmm_star(3, 4, False)
        sv, cards = [M1], (4,)
    elif name == "demo1-20":
        m, v, _ = tg.demo1(20)
        sv, cards = [v["A1"]], (20,)
    else:
        m, X1, O1, _ = tg.wide()
        sv, cards = [O1], (8,)
    liks = tg.weights(B, T, cards, 19)
    S, P = m.partial_size(), m.param_size()
    bp, partial = banded(S, torch.float64, -7.25)
    bl, ll = banded(B, torch.float64, -7.25)
    bs, status = banded(B, torch.int32, -7)
    p, _, st = run_partial(m, None, [], liks, sv, partial=partial, ll=ll, status=status)
    assert intact(bp, S, -7.25) and intact(bl, B, -7.25) and intact(bs, B, -7)
    assert np.all(st == 0) and np.isfinite(p).all() and p[-3:].tolist() == [0.0, 0.0, 1.0]
    bc, counts = banded(P, torch.float64, -7.25)
    counts.fill_(1.0)
    bl, ll = banded(B, torch.float64, -7.25)
    bs, status = banded(B, torch.int32, -7)
    c, _, st = run_counts(m, None, [], liks, sv, counts=counts, ll=ll, status=status)
    assert intact(bc, P, -7.25) and intact(bl, B, -7.25) and intact(bs, B, -7)
    assert np.all(st == 0) and np.all(c >= 1.0)


# ---------------------------------------------------------------------------
# 8. refusals

def refused(code, fn, *args):
    before = nip_amd.last_kernel()
    with pytest.raises(nip_amd.NipError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    assert nip_amd.last_kernel() == before                  # nothing was launched
    return str(e.value)


@pytest.mark.parametrize("fn", [nip_amd.estep_partial_soft, nip_amd.e_step_soft])
def test_refusals(fn):
    ones = lambda B, T, W: torch.ones((B, T, W), dtype=torch.float64, device="cuda")
    codes = lambda B, T, n: torch.zeros((B, T, n), dtype=torch.int32, device="cuda")
    f, cur, O1, _ = tg.factorial()
    assert "joint interface" in refused(UNSUPPORTED, fn, f, None, [], ones(2, 3, 5), [O1])
    m, P0, P1, M1, _ = hmm_star(3, 4, False)
    assert "interface variable itself" in refused(UNSUPPORTED, fn, m, None, [], ones(2, 3, 3), [P1])
    assert "interface variable itself" in refused(UNSUPPORTED, fn, m, codes(2, 3, 1), [P1], ones(2, 3, 4), [M1])
    assert "hard and as soft" in refused(UNSUPPORTED, fn, m, codes(2, 3, 1), [M1], ones(2, 3, 4), [M1])
    w, wP1, ov, _ = tg.five_children()
    assert "four" in refused(UNSUPPORTED, fn, w, codes(2, 3, 3), ov[:3], ones(2, 3, 4), ov[3:])
    refused(INVALID, fn, m, codes(2, 3, 1), [99], ones(2, 3, 4), [M1])
    refused(INVALID, fn, m, codes(2, 3, 1), [-1], None, [])
    refused(INVALID, fn, m, None, [], ones(2, 3, 4).cpu(), [M1])


# ---------------------------------------------------------------------------
# 9. em_learn_soft

def sample(A, pi, E, B, T, seed):
    """Codes [B, T] of the HMM's child, drawn from the tables (A[x][y], E[y][o])."""
    rng = np.random.default_rng(seed)
    draw = lambda p: (rng.random(p.shape[:-1] + (1,)) > np.cumsum(p / p.sum(axis=-1, keepdims=True), axis=-1)) \
        .sum(axis=-1).clip(max=p.shape[-1] - 1)
    x = draw(np.tile(pi, (B, 1)))
    out = np.zeros((B, T), np.int32)
    for t in range(T):
        x = draw(A[x])
        out[:, t] = draw(E[x])
    return out


def fresh_hmm(seed):
    """A model of its own: em_learn leaves its last m_step in it."""
    m = nip_amd.Model.from_spec(*synth.hmm_spec(4, 4, seed=seed, proper=True))
    return m, m.variable("M1")


EM_B, EM_T, EM_ITERS, THRESHOLD = 32, 24, 6, 1e-6


def test_em_learn_soft_on_one_hot_weights_is_em_learn():
    _, _, _, (A, pi, Es) = tg.hmm(4, 4, True, seed=1)
    codes = sample(A, pi, Es[0], EM_B, EM_T, 3)
    m, M1 = fresh_hmm(901)
    init = np.random.default_rng(4).random(m.param_size())
    hard, soft = [], []
    rc = nip_amd.em_learn(m, torch.from_numpy(codes[:, :, None]).cuda(), [M1], THRESHOLD, hard, init=init,
                          max_iterations=EM_ITERS)
    assert rc == 0 and len(hard) == EM_ITERS
    m2, M1 = fresh_hmm(901)
    _, w = dev(None, [], [es.one_hot(codes, 4)])
    rc = nip_amd.em_learn_soft(m2, None, [], w, [M1], THRESHOLD, soft, init=init, max_iterations=EM_ITERS)
    assert nip_amd.last_kernel() == KERNEL
    assert rc == 0 and len(soft) == EM_ITERS
    print("curves: hard %s soft %s" % (hard, soft))
    assert close(np.array(soft), np.array(hard), CURVE_RTOL)


def test_em_learn_soft_on_posterior_rows():
    """The lower model's smoothed rows of its interface, unchanged, as the
    upper HMM's child vectors: the curve does not decrease, and 2^10 times
    every vector moves it by 10 ln 2 per step."""
    low, P1, M1, (A, pi, Es) = tg.hmm(4, 4, True, seed=1)
    codes = sample(A, pi, Es[0], EM_B, EM_T, 5)
    rows, _, st = nip_amd.forward_backward_inference(low, torch.from_numpy(codes[:, :, None]).cuda(), [M1], [P1])
    assert np.all(st.cpu().numpy() == 0)
    rows = rows.contiguous()
    curves = []
    for scale in (1.0, 1024.0):
        up, U1 = fresh_hmm(902)
        init = np.random.default_rng(6).random(up.param_size())
        curve = []
        rc = nip_amd.em_learn_soft(up, None, [], rows * scale, [U1], THRESHOLD, curve, init=init,
                                   max_iterations=EM_ITERS)
        assert rc == 0 and len(curve) == EM_ITERS
        curves.append(np.array(curve))
    print("curves: %s, times 2^10 %s" % (curves[0], curves[1]))
    assert np.all(np.diff(curves[0]) >= -THRESHOLD)
    assert np.abs(curves[1] - curves[0] - 10 * LN2).max() <= 1e-9
