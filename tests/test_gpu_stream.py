"""Online inference on the GPU (nip_amd.Stream, nipamd_stream_*,
nip_amd/csrc/stream.hip chain_stream_kernel): resumable filtering and
fixed-lag smoothing of an interface chain.

The oracle is stream_util.fixed_lag -- plain numpy over the model's own tables,
pinned to the textbook smoother on every prefix by tests/test_stream_api.py.
Tolerances are the project's own (tests/test_gpu_filter.py,
tests/test_gpu_fb_ckw.py): rows 1e-12 absolute against the oracle, ll
1e-11 max(1, |ll|); against the existing GPU entry points rows 2e-12, the sum
of the two 1e-12 parity bounds.  Observations have 20 % missing.  Splits are
compared bit for bit.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import nip_amd
from nip_amd import synth

import stream_util as su
import viterbi_util as vu
from textbook_util import chain_tables

KERNEL = "chain_stream_kernel"
ROW_TOL, LL_TOL, GPU_TOL = 1e-12, 1e-11, 2e-12
CHUNK = nip_amd.STREAM_CHUNK


def gappy(B, T, cards, seed, frac=0.2):
    rng = np.random.default_rng(seed)
    obs = np.stack([rng.integers(0, c, size=(B, T)) for c in cards], axis=2).astype(np.int32) if cards \
        else np.zeros((B, T, 0), np.int32)
    obs[rng.random(obs.shape) < frac] = -1
    return obs


def feed(s, obs, splits, flush=True):
    """Push obs [B, T, n_obs] in pieces of `splits` steps, then flush: the
    rows in order [B, T (or the rows emitted), width], ll and status -- with
    the shape of every piece and the host counters checked after every call."""
    o = torch.from_numpy(np.ascontiguousarray(obs, np.int32)).cuda()
    assert sum(splits) == obs.shape[1]
    out, pos = [], 0
    for T in splits:
        pend = s.pending
        post = s.push(o[:, pos:pos + T].contiguous())
        assert nip_amd.last_kernel() == KERNEL
        pos += T
        assert tuple(post.shape) == (s.B, max(0, pend + T - s.lag), s.width)
        assert s.steps == pos and s.pending == min(pos, s.lag)
        out.append(post)
    if flush:
        pend = s.pending
        post = s.flush()
        assert tuple(post.shape) == (s.B, pend, s.width)
        assert s.steps == pos and s.pending == 0
        out.append(post)
    torch.cuda.synchronize()
    rows = torch.cat(out, dim=1).cpu().numpy()
    return rows, s.ll.cpu().numpy(), s.status.cpu().numpy()


def stream_rows(m, ov, q, obs, L, splits, flush=True):
    with nip_amd.Stream(m, ov, q, obs.shape[0], lag=L) as s:
        return feed(s, obs, splits, flush)


def check_ll(ll, want):
    err = np.abs(ll - want)
    bound = LL_TOL * np.maximum(1.0, np.abs(want))
    print("max |ll - oracle| %.3g (bound %.3g)" % (err.max(), bound.min()))
    assert np.all(err <= bound), err.max()


def check_rows(rows, want, tol, what="oracle"):
    assert rows.shape == want.shape, (rows.shape, want.shape)
    err = np.abs(rows - want).max()
    print("max |row - %s| %.3g (bound %.3g)" % (what, err, tol))
    assert err <= tol, err


# ---------------------------------------------------------------------------
# models, built once

@functools.lru_cache(maxsize=None)
def hmm(N, M, proper, seed=0):
    nodes, pots = synth.hmm_spec(N, M, seed=500 + N + seed, proper=proper)
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
def sticky(N):
    M = {3: 4, 16: 16, 20: 8, 64: 8}[N]
    m = nip_amd.Model.from_spec(*su.sticky_spec(N, M, 900 + N))
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    return m, P1, M1, M, chain_tables(m, P0, P1, [M1])


FILTER_CASES = {
    "hmm3": lambda: _hmm_case(3, 4, False), "hmm3-proper": lambda: _hmm_case(3, 4, True),
    "hmm16": lambda: _hmm_case(16, 16, False), "hmm16-proper": lambda: _hmm_case(16, 16, True),
    "demo1-17": lambda: _demo_case(17, "ab"), "demo1-20": lambda: _demo_case(20, "ab"),
    "demo1-32": lambda: _demo_case(32, "ab"), "demo1-33": lambda: _demo_case(33, "ab"),
    "demo1-20-one-column": lambda: _demo_case(20, "b"), "demo1-20-no-evidence": lambda: _demo_case(20, ""),
    "wide64-gpu-fold": lambda: _wide_case(),
}


def _hmm_case(N, M, proper):
    m, P1, M1, tables = hmm(N, M, proper)
    return m, [M1], [P1], (M,), tables, lambda obs: [obs[:, :, 0]]


def _demo_case(card, which):
    m, v, tables = demo1(card)
    ov = [v[c.upper() + "1"] for c in which]
    none = lambda obs: np.full(obs.shape[:2], -1)
    cols = {"ab": lambda obs: [obs[:, :, 0], obs[:, :, 1]], "b": lambda obs: [none(obs), obs[:, :, 0]],
            "": lambda obs: [none(obs), none(obs)]}[which]
    return m, ov, [v["C1"]], (card,) * len(which), tables, cols


def _wide_case():
    m, X1, O1, tables = wide()
    return m, [O1], [X1], (8,), tables, lambda obs: [obs[:, :, 0]]


# ---------------------------------------------------------------------------
# 1. filter parity

@pytest.mark.parametrize("B", [1, 5, 33])
@pytest.mark.parametrize("case", sorted(FILTER_CASES))
def test_filter_parity(case, B):
    """L = 0: the concatenated rows and the final ll / status against the
    oracle and against nipamd_filter one-shot; 70 steps fed as 1, 1, 2, 16, 17, 33."""
    m, ov, q, cards, (A, pi, Es), cols = FILTER_CASES[case]()
    T = 70
    obs = gappy(B, T, cards, 11 * B + len(case))
    rows, ll, st = stream_rows(m, ov, q, obs, 0, [1, 1, 2, 16, 17, 33])
    want, want_ll = su.fixed_lag(A, pi, Es, cols(obs), 0)
    check_rows(rows, want, ROW_TOL)
    check_ll(ll, want_ll)
    assert np.all(st == 0)
    post, fll, fst = nip_amd.forward_inference(m, torch.from_numpy(obs).cuda(), ov, q)
    torch.cuda.synchronize()
    check_rows(rows, post.cpu().numpy(), GPU_TOL, "nipamd_filter")
    check_ll(ll, fll.cpu().numpy())
    assert np.array_equal(st, fst.cpu().numpy())


# ---------------------------------------------------------------------------
# 2. fixed-lag parity on a model that remembers

T_LAG, B_LAG = 90, 5


@functools.lru_cache(maxsize=None)
def sticky_obs(N):
    return gappy(B_LAG, T_LAG, (sticky(N)[3],), 70 + N)


@functools.lru_cache(maxsize=None)
def sticky_reference(N, L):
    _, _, _, _, (A, pi, Es) = sticky(N)
    return su.fixed_lag(A, pi, Es, [sticky_obs(N)[:, :, 0]], L)


def lag_splits(L, total):
    """1, L - 1, L, L + 1, 3 and the rest (zero-length pushes dropped), cut where the total is reached."""
    out, left = [], total
    for T in [1, L - 1, L, L + 1, 3, total]:
        T = min(T, left)
        if T > 0:
            out.append(T)
            left -= T
    assert sum(out) == total
    return out


@pytest.mark.parametrize("N", [3, 16, 20, 64])
@pytest.mark.parametrize("L", [1, 2, 5, 15, 16, 17, 31, 32, 63, 64])
def test_fixed_lag_parity(N, L):
    m, P1, M1, M, _ = sticky(N)
    obs = sticky_obs(N)
    want, want_ll = sticky_reference(N, L)
    nxt, _ = sticky_reference(N, L + 1)
    # the rows whose endpoints differ between L and L + 1 must differ: an
    # endpoint off by one cannot pass
    differ = np.abs(want - nxt).max(axis=2)[:, :T_LAG - 1 - L]
    print("median |rows(L) - rows(L + 1)| %.3g" % np.median(differ))
    assert np.median(differ) >= 1e-4
    rows, ll, st = stream_rows(m, [M1], [P1], obs, L, lag_splits(L, T_LAG))
    check_rows(rows, want, ROW_TOL)
    check_ll(ll, want_ll)
    assert np.all(st == 0)


# ---------------------------------------------------------------------------
# 3. ends

def test_shorter_than_the_lag():
    """T_total < L: no push emits, the flush emits everything -- the smoothed rows."""
    m, P1, M1, (A, pi, Es) = hmm(16, 16, False)
    obs = gappy(5, 5, (16,), 31)
    with nip_amd.Stream(m, [M1], [P1], 5, lag=8) as s:
        o = torch.from_numpy(obs).cuda()
        for a, b in ((0, 2), (2, 5)):
            post = s.push(o[:, a:b].contiguous())
            assert tuple(post.shape) == (5, 0, 16)
            assert s.steps == b and s.pending == b
        rows = s.flush()
        assert s.pending == 0 and s.steps == 5
        torch.cuda.synchronize()
        want, want_ll = su.fixed_lag(A, pi, Es, [obs[:, :, 0]], 8)
        check_rows(rows.cpu().numpy(), want, ROW_TOL)
        check_ll(s.ll.cpu().numpy(), want_ll)


@pytest.mark.parametrize("proper", [False, True])
def test_lag_beyond_the_sequence_is_forward_backward(proper):
    """T_total = 40 under L = 64: pushes + flush are nipamd_fb's rows and ll."""
    m, P1, M1, (A, pi, Es) = hmm(16, 16, proper)
    obs = gappy(7, 40, (16,), 32)
    rows, ll, st = stream_rows(m, [M1], [P1], obs, 64, [7, 33])
    post, fll, fst = nip_amd.forward_backward_inference(m, torch.from_numpy(obs).cuda(), [M1], [P1])
    torch.cuda.synchronize()
    check_rows(rows, post.cpu().numpy(), GPU_TOL, "nipamd_fb")
    check_ll(ll, fll.cpu().numpy())
    assert np.array_equal(st, fst.cpu().numpy())
    want, want_ll = su.fixed_lag(A, pi, Es, [obs[:, :, 0]], 64)
    check_rows(rows, want, ROW_TOL)
    check_ll(ll, want_ll)


def test_push_after_flush_and_reset():
    m, P1, M1, _ = hmm(3, 4, False)
    obs = gappy(5, 20, (4,), 33)
    with nip_amd.Stream(m, [M1], [P1], 5, lag=3) as s:
        first = feed(s, obs, [4, 9, 7])
        with pytest.raises(nip_amd.NipError) as e:
            s.push(torch.from_numpy(obs[:, :2]).cuda().contiguous())
        assert e.value.code == nip_amd.NIP_ERROR_INVALID_ARGUMENT
        assert s.steps == 20 and s.pending == 0
        s.reset()
        assert s.steps == 0 and s.pending == 0
        again = feed(s, obs, [4, 9, 7])
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    assert first[0].shape == (5, 20, 3)


# ---------------------------------------------------------------------------
# 4. split invariance, bit for bit

def test_split_invariance():
    m, P1, M1, _ = hmm(16, 16, False)
    B, T, L = 33, 2 * CHUNK + 3, 5
    obs = gappy(B, T, (16,), 41)
    whole = stream_rows(m, [M1], [P1], obs, L, [T])
    assert whole[0].shape == (B, T, 16)
    for splits in ([1] * T, [CHUNK + 1, CHUNK + 2]):
        got = stream_rows(m, [M1], [P1], obs, L, splits)
        for a, b in zip(whole, got):
            assert np.array_equal(a, b), splits[:3]
    lo = stream_rows(m, [M1], [P1], obs[:16], L, [CHUNK + 1, CHUNK + 2])
    hi = stream_rows(m, [M1], [P1], obs[16:], L, [T])
    for a, x, y in zip(whole, lo, hi):
        assert np.array_equal(a, np.concatenate([x, y], axis=0))


# ---------------------------------------------------------------------------
# 5. a long stream

def test_long_stream():
    """1500 steps through pushes of 1, 7, 64, 128, ...: nothing underflows and
    nothing is rescaled away (the ll is the sum of 1500 step terms)."""
    m, P1, M1, (A, pi, Es) = hmm(16, 16, True)
    B, T, L = 5, 1500, 5
    obs = gappy(B, T, (16,), 51)
    splits, k = [], 0
    while sum(splits) < T:
        splits.append(min([1, 7, 64, 128][k % 4], T - sum(splits)))
        k += 1
    rows, ll, st = stream_rows(m, [M1], [P1], obs, L, splits)
    want, want_ll = su.fixed_lag(A, pi, Es, [obs[:, :, 0]], L)
    check_rows(rows, want, ROW_TOL)
    check_ll(ll, want_ll)
    assert np.all(st == 0) and np.all(ll < -1500.0)


# ---------------------------------------------------------------------------
# 6. joint interface

@functools.lru_cache(maxsize=None)
def factorial():
    nodes, pots = synth.factorial_spec(4, 4, 5, seed=61)
    m = nip_amd.Model.from_spec(nodes, pots)
    d = m.desc()
    cur, prev = d["outgoing"], d["previous_outgoing"]
    O1 = m.variable("O1")
    return m, cur, O1, vu.joint_tables(m, prev, cur, O1)


@pytest.mark.parametrize("L", [0, 3])
def test_joint_interface(L):
    m, cur, O1, (A, pi, E) = factorial()
    X1, Y1 = m.variable("X1"), m.variable("Y1")
    stride = {cur[0]: 1, cur[1]: m.card(cur[0])}
    obs = gappy(9, 30, (5,), 61)
    joint, want_ll = su.fixed_lag(A, pi, [E], [obs[:, :, 0]], L)
    wx, wy = su.digit_sums(joint, stride[X1], 4), su.digit_sums(joint, stride[Y1], 4)
    xy, ll, st = stream_rows(m, [O1], [X1, Y1], obs, L, [4, 11, 15])
    assert xy.shape == (9, 30, 8)
    check_rows(xy, np.concatenate([wx, wy], axis=2), ROW_TOL)
    check_ll(ll, want_ll)
    assert np.all(st == 0)
    yx, ll2, st2 = stream_rows(m, [O1], [Y1, X1], obs, L, [4, 11, 15])
    assert np.array_equal(yx[:, :, :4], xy[:, :, 4:]) and np.array_equal(yx[:, :, 4:], xy[:, :, :4])
    assert np.array_equal(ll2, ll) and np.array_equal(st2, st)
    y, ll3, _ = stream_rows(m, [O1], [Y1], obs, L, [30])
    assert y.shape == (9, 30, 4)
    assert np.array_equal(y, xy[:, :, 4:]) and np.array_equal(ll3, ll)


# ---------------------------------------------------------------------------
# 7. evidence on the interface variable

def test_evidence_on_the_interface_variable():
    m, P1, M1, (A, pi, Es) = hmm(16, 16, False)
    B, T, L = 9, 40, 2
    rng = np.random.default_rng(8)
    obs = gappy(B, T, (16, 16), 17)
    seen = rng.random((B, T)) < 0.5
    obs[:, :, 1] = np.where(seen, rng.integers(0, 16, size=(B, T)), -1)
    rows, ll, st = stream_rows(m, [M1, P1], [P1], obs, L, [3, 20, 17])
    want, want_ll = su.fixed_lag(A, pi, Es + [np.eye(16)], [obs[:, :, 0], obs[:, :, 1]], L)
    check_rows(rows, want, ROW_TOL)
    check_ll(ll, want_ll)
    assert np.all(st == 0)
    assert np.array_equal(rows[seen], np.eye(16)[obs[:, :, 1][seen]])


# ---------------------------------------------------------------------------
# 8. zero mass is per sequence

def test_zero_mass_is_per_sequence():
    m, P1, M1, _ = hmm(3, 4, False)
    B, T, L = 5, 23, 3
    obs = gappy(B, T, (4,), 6)
    good = stream_rows(m, [M1], [P1], obs, L, [4, 6, 13])
    bad = obs.copy()
    bad[2, 9, 0] = 4                                           # == M: out of range, no mass at step 9
    rows, ll, st = stream_rows(m, [M1], [P1], bad, L, [4, 6, 13])
    assert st[2] & nip_amd.STATUS_ZERO_MASS and ll[2] == -vu.DBL_MAX
    assert np.all(rows[2, 6:] == 0.0)                          # min(t + 3, 22) >= 9
    assert np.array_equal(rows[2, :6], good[0][2, :6])
    keep = [0, 1, 3, 4]
    assert np.array_equal(rows[keep], good[0][keep])
    assert np.array_equal(ll[keep], good[1][keep]) and np.all(st[keep] == 0)
    _, fll, fst = nip_amd.forward_inference(m, torch.from_numpy(bad).cuda(), [M1], [P1])
    torch.cuda.synchronize()
    fll, fst = fll.cpu().numpy(), fst.cpu().numpy()
    assert np.array_equal(st, fst) and fll[2] == ll[2]
    check_ll(ll[keep], fll[keep])
    # the status is sticky and the dead step is remembered across pushes: single steps give the same bits
    single = stream_rows(m, [M1], [P1], bad, L, [1] * T)
    for a, b in zip((rows, ll, st), single):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------
# 9. buffers and forms

def test_callers_buffers_and_stream():
    m, P1, M1, _ = hmm(16, 16, False)
    B, L = 13, 4
    obs = gappy(B, 30, (16,), 4)
    want = stream_rows(m, [M1], [P1], obs, L, [10, 20])
    o = torch.from_numpy(obs).cuda()
    hs = torch.cuda.Stream()
    hs.wait_stream(torch.cuda.current_stream())
    with nip_amd.Stream(m, [M1], [P1], B, lag=L) as s, torch.cuda.stream(hs):
        p1 = torch.full((B, 6, 16), -7.0, dtype=torch.float64, device="cuda")
        p2 = torch.full((B, 20, 16), -7.0, dtype=torch.float64, device="cuda")
        p3 = torch.full((B, 4, 16), -7.0, dtype=torch.float64, device="cuda")
        assert s.push(o[:, :10].contiguous(), post=p1, stream=hs) is p1
        assert s.push(o[:, 10:].contiguous(), post=p2, stream=hs) is p2
        assert s.flush(post=p3, stream=hs) is p3
        hs.synchronize()
        assert np.array_equal(torch.cat([p1, p2, p3], dim=1).cpu().numpy(), want[0])
        assert np.array_equal(s.ll.cpu().numpy(), want[1]) and np.array_equal(s.status.cpu().numpy(), want[2])
        s.reset(stream=hs)
        with pytest.raises(nip_amd.NipError):
            s.push(o[:, :10].contiguous(), post=torch.zeros((B, 6, 16), device="cuda"))            # float32
        with pytest.raises(nip_amd.NipError):
            s.push(o[:, :10].contiguous(), post=torch.zeros((B, 7, 16), dtype=torch.float64, device="cuda"))
        with pytest.raises(nip_amd.NipError):
            s.push(o[:5, :10].contiguous())                                                       # another B
        with pytest.raises(nip_amd.NipError):
            s.push(o[:, :10].to(torch.int64))
        assert s.steps == 0
    with pytest.raises(nip_amd.NipError):
        s.push(o[:, :10].contiguous())                                                            # closed


def test_host_form_is_the_device_form():
    m, P1, M1, _ = hmm(3, 4, True)
    B, L = 6, 2
    obs = gappy(B, 21, (4,), 12)
    want = stream_rows(m, [M1], [P1], obs, L, [1, 8, 12])
    with nip_amd.Stream(m, [M1], [P1], B, lag=L) as s:
        out = []
        for a, b in ((0, 1), (1, 9), (9, 21)):
            post, ll, st = s.push_host(obs[:, a:b])
            assert post.shape == (B, max(0, min(a, L) + (b - a) - L), 3)
            out.append(post)
        post, ll, st = s.flush_host()
        out.append(post)
        assert s.steps == 21 and s.pending == 0
    assert np.array_equal(np.concatenate(out, axis=1), want[0])
    assert np.array_equal(ll, want[1]) and np.array_equal(st.astype(np.int32), want[2])
