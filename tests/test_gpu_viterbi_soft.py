"""most_likely_states_soft / nipamd_mlss_soft on the GPU
(nip_amd/csrc/viterbi_soft.hip, chain_viterbi_soft_kernel): the most likely
sequence of the interface under hard and soft (likelihood) evidence.

The oracle is viterbi_soft_util.viterbi_soft -- viterbi_util's recursion with
soft_util's step evidence, pinned to its brute force by
tests/test_viterbi_soft_api.py.  Per batch, tests/test_gpu_viterbi.py's rule
with its values:

 (a) every state is within its variable's cardinality;
 (b) the GPU path's own score under the weights as given (path_score_soft) is
     at least the oracle's optimum - 1e-11 max(1, |optimum|), and logp is
     within the same bound of the optimum;
 (c) at most 10 % of a batch's sequences have a path differing anywhere from
     the oracle's.  tests/test_viterbi_soft_api.py shows on these very inputs
     (viterbi_soft_util builds them for both files) that rounding alone -- the
     fp64 against the long double recursion -- moves at most 2 %.

Weights are 0.05 + U[0, 1) and hard columns have 20 % missing unless a test
says otherwise.  Exact scalings, batch independence, caller's buffers and the
host form are compared bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import nip_amd

import soft_scale_util as ssu
import soft_util as so
import test_gpu_soft as tg
import viterbi_soft_util as vsu
import viterbi_util as vu

KERNEL = "chain_viterbi_soft_kernel"
TOL = 1e-11
DEAD = nip_amd.STATUS_ZERO_MASS | nip_amd.STATUS_BAD_EVIDENCE


def gpu(m, obs, ov, liks, sv, q, **kw):
    """The device call: obs [B, T, n_obs] int32 (or None), liks the soft
    columns' weight arrays in sv order.  Numpy (path, logp, status)."""
    o = torch.from_numpy(np.ascontiguousarray(obs, np.int32)).cuda() if obs is not None and len(ov) else None
    w = torch.from_numpy(np.ascontiguousarray(np.concatenate(liks, axis=2))).cuda() if liks else None
    path, logp, st = nip_amd.most_likely_states_soft(m, o, ov, w, sv, q, **kw)
    assert nip_amd.last_kernel() == KERNEL
    torch.cuda.synchronize()
    return path.cpu().numpy(), logp.cpu().numpy(), st.cpu().numpy()


def run(r, obs, liks, q=None):
    return gpu(r.m, obs, r.ov, liks, r.sv, r.q if q is None else q)


def hard(m, obs, ov, q):
    path, logp, st = nip_amd.most_likely_states(m, torch.from_numpy(np.ascontiguousarray(obs, np.int32)).cuda(), ov, q)
    torch.cuda.synchronize()
    return path.cpu().numpy(), logp.cpu().numpy(), st.cpu().numpy()


def bound_of(opt):
    return TOL * np.maximum(1.0, np.abs(opt))


def check(r, obs, liks, got, what=""):
    """(a), (b), (c) of one batch against the oracle; returns the oracle's path."""
    path, logp, st = got
    want, opt, want_st = vsu.oracle(r, obs, liks)
    assert np.all(want_st == 0), "the case is meant to have mass everywhere"
    assert np.all(st == 0)
    B, T = want.shape
    assert path.shape == (B, T, len(r.q)) and path.dtype == np.int32
    cards = [c for _, c in r.digits] if r.digits else [r.tables[0].shape[0]]
    for j, c in enumerate(cards):
        assert path[:, :, j].min() >= 0 and path[:, :, j].max() < c                 # (a)
    joint = vsu.joint_state(r, path)
    score = vsu.score(r, obs, liks, joint)
    bound = bound_of(opt)
    differ = int((joint != want).any(axis=1).sum())
    print("%s %s: max optimum - score %.3g, max |logp - optimum| %.3g (bound %.3g); paths differing from the "
          "oracle's: %d / %d" % (r.name, what, (opt - score).max(), np.abs(logp - opt).max(), bound.min(), differ, B))
    assert np.all(score >= opt - bound), (opt - score).max()                        # (b)
    assert np.all(np.abs(logp - opt) <= bound), np.abs(logp - opt).max()
    assert differ <= 0.10 * B, (differ, B)                                          # (c)
    return want


# ---------------------------------------------------------------------------
# 1. every kernel variant at its smallest shape

@pytest.mark.parametrize("T", ssu.TS)
@pytest.mark.parametrize("name", ssu.NAMES)
def test_every_variant(name, T):
    """NP 16 / 32 / 64, a vector longer than the group, no hard column and one
    beside a soft one, 2 and 4 soft columns, a joint interface's digits."""
    r, obs, liks = vsu.grid_case(name, T)
    got = run(r, obs, liks)
    check(r, obs, liks, got)
    if name == "factorial-yx":
        swapped = run(r, obs, liks, q=r.q[::-1])
        assert np.array_equal(swapped[0], got[0][:, :, ::-1])
        assert np.array_equal(swapped[1], got[1]) and np.array_equal(swapped[2], got[2])


# ---------------------------------------------------------------------------
# 2. the kernel's periods

@pytest.mark.parametrize("name,B,T", vsu.PERIODS)
def test_periods(name, B, T):
    r, obs, liks = vsu.period_case(name, B, T)
    check(r, obs, liks, run(r, obs, liks), "B=%d T=%d" % (B, T))


# ---------------------------------------------------------------------------
# 3., 4. against most_likely_states

def _parity_case(name):
    r = vsu.requests()["hmm16" if name == "hmm16" else "demo20-both"]
    cards = ssu.cards(r, r.soft)
    return r, cards, tg.gappy(5, 40, cards, 31 + len(name), frac=0.0)


def one_hot(codes, card):
    return np.eye(card)[codes]


def same_logp(logp, want):
    assert np.all(np.abs(logp - want) <= bound_of(want)), np.abs(logp - want).max()


@pytest.mark.parametrize("name", ["hmm16", "demo20"])
def test_one_hot_weights_are_hard_observations(name):
    r, cards, obs = _parity_case(name)
    want = hard(r.m, obs, r.sv, r.q)
    got = gpu(r.m, None, [], [one_hot(obs[:, :, k], c) for k, c in enumerate(cards)], r.sv, r.q)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    same_logp(got[1], want[1])
    if len(cards) == 2:                                      # one column hard, the other one-hot
        got = gpu(r.m, obs[:, :, 1:], r.sv[1:], [one_hot(obs[:, :, 0], cards[0])], r.sv[:1], r.q)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
        same_logp(got[1], want[1])
    got = gpu(r.m, obs, r.sv, [], [], r.q)                   # no soft column at all
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    same_logp(got[1], want[1])


@pytest.mark.parametrize("name", ["hmm16", "demo20"])
def test_all_ones_weights_are_a_missing_column(name):
    r, cards, obs = _parity_case(name)
    B, T = obs.shape[:2]
    if len(cards) == 1:
        empty = torch.empty((B, T, 0), dtype=torch.int32, device="cuda")
        _, want, st = nip_amd.most_likely_states(r.m, empty, [], r.q)
        torch.cuda.synchronize()
        want, st = want.cpu().numpy(), st.cpu().numpy()
        got = gpu(r.m, None, [], [np.ones((B, T, cards[0]))], r.sv, r.q)
    else:
        _, want, st = hard(r.m, obs[:, :, 1:], r.sv[1:], r.q)
        got = gpu(r.m, obs[:, :, 1:], r.sv[1:], [np.ones((B, T, cards[0]))], r.sv[:1], r.q)
    assert np.all(st == 0) and np.all(got[2] == 0)
    same_logp(got[1], want)


# ---------------------------------------------------------------------------
# 5. weights at every scale

@pytest.mark.parametrize("big", [560, 530])
@pytest.mark.parametrize("T", ssu.TS)
@pytest.mark.parametrize("name", ssu.NAMES)
def test_an_exact_scaling_moves_only_logp(name, T, big):
    r, obs, base = vsu.grid_case(name, T)
    k = ssu.exponents(T, len(r.soft), big)
    liks = ssu.scaled(base, k)
    control = run(r, obs, base)
    got = run(r, obs, liks)
    assert np.array_equal(got[0], control[0]) and np.array_equal(got[2], control[2])
    shift = k.sum(axis=(1, 2)) * vu.LN2
    excess = np.abs(got[1] - control[1] - shift)
    print("max |logp_scaled - logp_control - ksum ln 2| %.3g" % excess.max())
    assert np.all(excess <= bound_of(got[1]))
    check(r, obs, liks, got, "big=%d" % big)


@pytest.mark.parametrize("T", ssu.TS)
@pytest.mark.parametrize("name", ssu.NAMES)
def test_edge_weights(name, T):
    """Entries 2^-600 apart, all-denormal vectors, DBL_MAX: against the oracle."""
    r, obs, liks = vsu.edge_case(name, T)
    check(r, obs, liks, run(r, obs, liks), "edge")


# ---------------------------------------------------------------------------
# 6. bad weights and dead sequences are per sequence

@pytest.mark.parametrize("piece", [3, 18])
def test_bad_weights_are_per_sequence(piece):
    """A 20-state child on a 16-lane group: weight 3 is in the vector's first
    piece, weight 18 in the one the kernel loads on demand."""
    r, obs, liks = vsu.grid_case("hmm3x20-long", 24)
    good = run(r, obs, liks)
    assert np.all(good[2] == 0)
    bad = liks[0].copy()
    bad[1, 9, piece] = np.nan
    bad[3, 0, piece] = -1.0
    bad[4, 23, piece] = np.inf
    bad[6, 11] = 0.0
    path, logp, st = run(r, obs, [bad])
    assert list(st) == [0, DEAD, 0, DEAD, DEAD, 0, nip_amd.STATUS_ZERO_MASS]
    for b in (1, 3, 4, 6):
        assert np.all(path[b] == -1) and logp[b] == -vu.DBL_MAX
    assert not np.isnan(logp).any()
    keep = [0, 2, 5]
    assert np.array_equal(path[keep], good[0][keep]) and np.array_equal(logp[keep], good[1][keep])
    want = vsu.oracle(r, obs, [bad])
    assert np.array_equal(want[2], st) and np.all(want[0][[1, 3, 4, 6]] == -1)


def test_batch_independence():
    r, obs, liks = vsu.period_case("demo33-a-soft-b-hard", 5, 21)
    whole = run(r, obs, liks)
    rev = run(r, obs[::-1], [w[::-1] for w in liks])
    for a, b in zip(whole, rev):
        assert np.array_equal(a, b[::-1])
    alone = run(r, obs[2:3], [w[2:3] for w in liks])
    for a, b in zip(whole, alone):
        assert np.array_equal(a[2:3], b)


# ---------------------------------------------------------------------------
# 7., 8., 9.

def test_brute_force():
    """All 729 paths of every sequence: the GPU path's score under the weights
    as given, and logp, are the enumerated maximum."""
    N, M, B, T = vsu.BRUTE
    m, P1, M1, (A, pi, Es) = tg.hmm(N, M, False)
    rng = np.random.default_rng(77)
    w = np.ldexp(0.05 + rng.random((B, T, M)), rng.integers(-40, 41, size=(B, T, 1)))
    path, logp, st = gpu(m, None, [], [w], [M1], [P1])
    assert np.all(st == 0)
    args = ([so.SOFT], [None], [w])
    score = vsu.path_score_soft(A, pi, Es, *args, path[:, :, 0].astype(np.int64))
    for b in range(B):
        best, _ = vsu.brute_force_soft(A, pi, Es, *args, b)
        assert abs(score[b] - best) <= TOL * max(1.0, abs(best))
        assert abs(logp[b] - best) <= TOL * max(1.0, abs(best))


def test_long_sequence_rescaling():
    """T = 4097: delta underflows after a few hundred steps unless the
    exponents are carried."""
    r, obs, liks = vsu.long_case()
    got = run(r, obs, liks)
    assert np.all(got[1] < -4097.0)
    check(r, obs, liks, got, "T=4097")


def test_posterior_rows_fed_back_as_evidence():
    """The rows nipamd_fb writes for [P1] of one model are the likelihood rows
    of the interface variable of a second one, unchanged, beside its child's
    hard codes."""
    (m1, ov1, q1, _, codes1), r2, obs2 = vsu.fed_case()
    post, _, _ = nip_amd.forward_backward_inference(m1, torch.from_numpy(codes1).cuda(), ov1, q1)
    o = torch.from_numpy(obs2).cuda()
    path, logp, st = nip_amd.most_likely_states_soft(r2.m, o, r2.ov, post, r2.sv, r2.q)
    assert nip_amd.last_kernel() == KERNEL
    torch.cuda.synchronize()
    check(r2, obs2, [post.cpu().numpy()], (path.cpu().numpy(), logp.cpu().numpy(), st.cpu().numpy()))


# ---------------------------------------------------------------------------
# 10. the caller's buffers, the host form

def test_callers_buffers_and_stream():
    r, obs, liks = vsu.grid_case("demo20-a-soft-b-hard", 24)
    want = run(r, obs, liks)
    B, T = obs.shape[:2]
    path = torch.full((B, T, 1), -7, dtype=torch.int32, device="cuda")
    logp = torch.zeros(B, dtype=torch.float64, device="cuda")
    st = torch.full((B,), 9, dtype=torch.int32, device="cuda")
    o, w = torch.from_numpy(obs).cuda(), torch.from_numpy(liks[0]).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = nip_amd.most_likely_states_soft(r.m, o, r.ov, w, r.sv, r.q, path=path, logp=logp, status=st, stream=s)
    s.synchronize()
    assert nip_amd.last_kernel() == KERNEL
    assert got[0] is path and got[1] is logp and got[2] is st
    for g, x in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), x)
    with pytest.raises(nip_amd.NipError):
        nip_amd.most_likely_states_soft(r.m, o, r.ov, w, r.sv, r.q, path=torch.zeros((B, T, 1), device="cuda"))
    for bad in (w.float(), w[:, :, :3].contiguous(), w.cpu(), None):
        with pytest.raises(nip_amd.NipError) as e:
            nip_amd.most_likely_states_soft(r.m, o, r.ov, bad, r.sv, r.q)
        assert e.value.code == nip_amd.NIP_ERROR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", ["demo20-a-soft-b-hard", "factorial-yx"])
def test_host_form_is_the_device_form(name):
    r, obs, liks = vsu.grid_case(name, 24)
    want = run(r, obs, liks)
    path, logp, st = nip_amd.most_likely_states_soft_host(r.m, obs if r.ov else None, r.ov, liks[0], r.sv, r.q)
    assert nip_amd.last_kernel() == KERNEL
    assert path.dtype == np.int32 and path.shape == want[0].shape
    assert np.array_equal(path, want[0]) and np.array_equal(logp, want[1])
    assert np.array_equal(st.astype(np.int32), want[2])
