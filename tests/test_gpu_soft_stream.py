"""Online inference under soft evidence on the GPU (nip_amd.Stream with
soft_vars, nipamd_stream_open_soft / nipamd_stream_push_soft,
nip_amd/csrc/stream_soft.hip chain_stream_soft_kernel).

The oracle is soft_stream_util.soft_fixed_lag -- plain numpy over the model's
own tables, pinned to soft_util.soft_smoother and stream_util.fixed_lag by
tests/test_soft_stream_api.py.  Tolerances are the project's own
(tests/test_gpu_stream.py, tests/test_gpu_soft.py): rows 1e-12 absolute against
the oracle, ll 1e-11 max(1, |ll|); against another GPU entry point rows 2e-12.
Models are tests/test_gpu_soft.py's cached builders through
soft_scale_util.requests(): the smallest shape that reaches each path of the
kernel.  Weights are 0.05 + U[0, 1) and hard columns have 20 % missing unless a
test says otherwise.  Splits, batch splits and the host forms are compared bit
for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import nip_amd

import soft_scale_util as scu
import soft_stream_util as ssu
import soft_util as so
import test_gpu_soft as tg
from viterbi_util import DBL_MAX, LN2

KERNEL = "chain_stream_soft_kernel"
HARD_KERNEL = "chain_stream_kernel"
ROW_TOL, LL_TOL, GPU_TOL = tg.ROW_TOL, tg.LL_TOL, tg.GPU_TOL
CHUNK = nip_amd.STREAM_CHUNK
SPLITS = (1, 2, 64, 65, 18)                                  # 150 steps; 65 is two launches
T_ALL = sum(SPLITS)
BAD = nip_amd.STATUS_BAD_EVIDENCE | nip_amd.STATUS_ZERO_MASS


@functools.lru_cache(maxsize=None)
def requests():
    """soft_scale_util's requests, demo1(33) (NP = 64) and soft evidence on the
    interface variable of hmm(3, 4)."""
    out = dict(scu.requests())
    m, v, tables = tg.demo1(33)
    out["demo33-a-soft-b-hard"] = scu.Req("demo33-a-soft-b-hard", m, tables, (0,), (1,), [v["A1"]], [v["B1"]],
                                          [v["C1"]], None)
    m, P1, M1, (A, pi, Es) = tg.hmm(3, 4, False)
    out["hmm3-interface"] = scu.Req("hmm3-interface", m, (A, pi, Es + [np.eye(3)]), (1,), (), [P1], [], [P1], None)
    return out


def inputs(r, B, T, seed):
    """(obs [B, T, n_hard] int32, one [B, T, M] weight array per soft column)."""
    return tg.gappy(B, T, scu.cards(r, r.hard), 100 + seed), tg.weights(B, T, scu.cards(r, r.soft), 200 + seed)


def cuda(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def feed(s, obs, liks, splits, flush=True, kernel=KERNEL, trace=None):
    """Push the steps in pieces of `splits`, then flush: the rows in order
    [B, T (or the rows emitted), width], ll and status -- with the shape of
    every piece and the host counters checked after every call.  trace: a list
    that receives (ll, status) after every call."""
    o = cuda(obs, np.int32) if s.obs_vars else None
    w = cuda(np.concatenate(liks, axis=2), np.float64) if liks else None
    assert sum(splits) == (liks[0] if liks else obs).shape[1]

    def seen():
        if trace is not None:
            torch.cuda.synchronize()
            trace.append((s.ll.cpu().numpy().copy(), s.status.cpu().numpy().copy()))

    out, pos = [], 0
    for T in splits:
        pend = s.pending
        post = s.push(None if o is None else o[:, pos:pos + T].contiguous(),
                      lik=None if w is None else w[:, pos:pos + T].contiguous())
        assert nip_amd.last_kernel() == kernel
        pos += T
        assert tuple(post.shape) == (s.B, max(0, pend + T - s.lag), s.width)
        assert s.steps == pos and s.pending == min(pos, s.lag)
        out.append(post)
        seen()
    if flush:
        pend = s.pending
        post = s.flush()
        assert nip_amd.last_kernel() == kernel
        assert tuple(post.shape) == (s.B, pend, s.width)
        assert s.steps == pos and s.pending == 0
        out.append(post)
        seen()
    torch.cuda.synchronize()
    rows = torch.cat(out, dim=1).cpu().numpy()
    return rows, s.ll.cpu().numpy(), s.status.cpu().numpy()


def stream_rows(r, obs, liks, L, splits, flush=True, trace=None):
    B = (liks[0] if liks else obs).shape[0]
    with nip_amd.Stream(r.m, r.ov, r.q, B, lag=L, soft_vars=r.sv) as s:
        return feed(s, obs, liks, splits, flush, trace=trace)


def oracle(r, obs, liks, L):
    """(rows, ll, status) in the query's layout."""
    A, pi, Es = r.tables
    rows, ll, st = ssu.soft_fixed_lag(A, pi, Es, *scu.oracle_args(r, obs, liks), L)
    return scu.query_rows(r, rows), ll, st


def check(got, want):
    tg.check_rows(got[0], want[0], ROW_TOL)
    tg.check_ll(got[1], want[1])
    assert np.array_equal(got[2], want[2]), (got[2], want[2])


def same_bits(a, b, what=""):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


# ---------------------------------------------------------------------------
# 1. against the oracle

PARITY = ["hmm16", "hmm16-proper", "hmm3x20-long", "demo20-both", "demo20-a-soft-b-hard", "demo33-a-soft-b-hard",
          "wide64", "five-children-4-soft", "factorial-yx", "hmm3-interface"]


@pytest.mark.parametrize("L", [0, 5])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("name", PARITY)
def test_oracle_parity(name, B, L):
    """150 steps as 1, 2, 64, 65, 18 and a flush; B = 5 leaves the last wave
    part empty at every NP; at L = 5 the ring of 69 slots wraps twice."""
    r = requests()[name]
    obs, liks = inputs(r, B, T_ALL, 7 * B + len(name))
    got = stream_rows(r, obs, liks, L, SPLITS)
    assert got[0].shape[:2] == (B, T_ALL)
    want = oracle(r, obs, liks, L)
    assert np.all(want[2] == 0)
    check(got, want)


@pytest.mark.parametrize("L", [1, 15, 16, 17, 63, 64])
@pytest.mark.parametrize("name", ["hmm16", "demo20-both"])
def test_lag_sweep(name, L):
    r = requests()[name]
    obs, liks = inputs(r, 5, T_ALL, L + len(name))
    check(stream_rows(r, obs, liks, L, SPLITS), oracle(r, obs, liks, L))


def test_the_ring_wraps_three_times():
    """400 steps at L = 64: R = 128 slots."""
    r = requests()["hmm16"]
    obs, liks = inputs(r, 5, 400, 3)
    check(stream_rows(r, obs, liks, 64, (7, 64, 128, 1, 130, 70)), oracle(r, obs, liks, 64))


# ---------------------------------------------------------------------------
# 2. against the existing entry points

def soft_entry(which, r, obs, liks):
    return tg.run(which, r.m, obs if r.ov else None, r.ov, liks, r.sv, r.q)


@pytest.mark.parametrize("name", ["hmm16", "demo20-a-soft-b-hard", "factorial-yx"])
def test_lag_0_is_filter_soft(name):
    r = requests()[name]
    obs, liks = inputs(r, 5, 70, 11)
    rows, ll, st = stream_rows(r, obs, liks, 0, (70,))
    post, fll, fst = soft_entry(tg.FILTER, r, obs, liks)
    tg.check_rows(rows, post, GPU_TOL, "nipamd_filter_soft")
    tg.check_ll(ll, fll)
    assert np.array_equal(st, fst)


@pytest.mark.parametrize("name", ["hmm16", "hmm16-proper", "demo20-a-soft-b-hard"])
def test_lag_beyond_the_stream_is_fb_soft(name):
    """T = 40 under L = 64: a push and a flush; no push emits (a stream shorter than its lag)."""
    r = requests()[name]
    obs, liks = inputs(r, 5, 40, 12)
    rows, ll, st = stream_rows(r, obs, liks, 64, (40,))
    post, fll, fst = soft_entry(tg.FB, r, obs, liks)
    tg.check_rows(rows, post, GPU_TOL, "nipamd_fb_soft")
    tg.check_ll(ll, fll)
    assert np.array_equal(st, fst)


def hard_stream(m, ov, q, obs, L, splits, soft_vars=None):
    """The hard Stream (soft_vars None: the constructor's default)."""
    kw = {} if soft_vars is None else {"soft_vars": soft_vars}
    with nip_amd.Stream(m, ov, q, obs.shape[0], lag=L, **kw) as s:
        return feed(s, obs, [], splits, kernel=HARD_KERNEL)


@pytest.mark.parametrize("L", [0, 5])
@pytest.mark.parametrize("name", ["hmm16", "demo20-both"])
def test_one_hot_and_all_ones_weights_are_the_hard_stream(name, L):
    """An observed code as a one-hot vector, a missing one as all ones."""
    r = requests()[name]
    B, T = 5, 70
    cards = scu.cards(r, r.soft)
    obs = tg.gappy(B, T, cards, 21 + L)
    liks = []
    for k, c in enumerate(cards):
        w = np.eye(c)[np.maximum(obs[:, :, k], 0)]
        w[obs[:, :, k] < 0] = 1.0
        liks.append(w)
    rows, ll, st = stream_rows(r, None, liks, L, (3, 64, 3))
    want = hard_stream(r.m, r.sv, r.q, obs, L, (3, 64, 3))
    tg.check_rows(rows, want[0], GPU_TOL, "the hard stream")
    tg.check_ll(ll, want[1])
    assert np.array_equal(st, want[2])


def test_no_soft_columns_is_the_hard_stream():
    """soft_vars=() in Python, and n_soft == 0 with d_lik == NULL through the C
    ABI: chain_stream_kernel and its bits."""
    m, P1, M1, _ = tg.hmm(16, 16, False)
    B, T, L = 5, 70, 5
    obs = tg.gappy(B, T, (16,), 23)
    want = hard_stream(m, [M1], [P1], obs, L, (3, 64, 3))
    same_bits(hard_stream(m, [M1], [P1], obs, L, (3, 64, 3), soft_vars=()), want)
    lib = nip_amd.lib()
    h = C.c_void_p()
    assert lib.nipamd_stream_open_soft(m._h, 1, nip_amd._ints([M1]), 0, None, 1, nip_amd._ints([P1]), B, L,
                                       C.byref(h)) == 0
    try:
        o = cuda(obs, np.int32)
        post = torch.zeros((B, T - L, 16), dtype=torch.float64, device="cuda")
        tail = torch.zeros((B, L, 16), dtype=torch.float64, device="cuda")
        ll = torch.zeros((B,), dtype=torch.float64, device="cuda")
        st = torch.zeros((B,), dtype=torch.int32, device="cuda")
        ptr = lambda t: C.c_void_p(t.data_ptr())
        assert lib.nipamd_stream_push_soft(h, ptr(o), None, T, ptr(post), ptr(ll), ptr(st), None) == 0
        assert nip_amd.last_kernel() == HARD_KERNEL
        assert lib.nipamd_stream_flush(h, ptr(tail), ptr(ll), ptr(st), None) == 0
        torch.cuda.synchronize()
        same_bits((torch.cat([post, tail], dim=1).cpu().numpy(), ll.cpu().numpy(), st.cpu().numpy()), want)
    finally:
        lib.nipamd_stream_free(h)


# ---------------------------------------------------------------------------
# 3. split and batch invariance, bit for bit

@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "pattern-6"])
@pytest.mark.parametrize("name", ["hmm16", "demo20-a-soft-b-hard"])
def test_split_and_batch_invariance(name, scaled):
    r = requests()[name]
    B, L = 5, 5
    obs, liks = inputs(r, B, T_ALL, 31)
    if scaled:                                               # random exponents in [-900, 900] per step and column
        k = np.broadcast_to(scu.exponents(T_ALL, len(r.soft))[6], (B, T_ALL, len(r.soft)))
        liks = scu.scaled(liks, k)
    cut = lambda b: (obs[b], [w[b] for w in liks])
    whole = stream_rows(r, obs, liks, L, (T_ALL,))
    assert whole[0].shape[:2] == (B, T_ALL) and np.all(whole[2] == 0)
    same_bits(stream_rows(r, obs, liks, L, (1,) * T_ALL), whole, "150 pushes of 1")
    same_bits(stream_rows(r, obs, liks, L, SPLITS), whole, SPLITS)
    lo, hi = stream_rows(r, *cut(slice(0, 2)), L, SPLITS), stream_rows(r, *cut(slice(2, 5)), L, (T_ALL,))
    same_bits([np.concatenate([x, y], axis=0) for x, y in zip(lo, hi)], whole, "streams of 2 + 3")
    rev = stream_rows(r, *cut(slice(None, None, -1)), L, SPLITS)
    same_bits([x[::-1] for x in rev], whole, "the batch reversed")


# ---------------------------------------------------------------------------
# 4. weight scales

T_SCALE, SCALE_SPLITS = 37, (10, 27)
GRID = [(name, 560) for name in scu.NAMES] + [(name, 530) for name in scu.TWO_COLUMN]


@functools.lru_cache(maxsize=None)
def scale_base(name, L):
    r = scu.requests()[name]
    obs, base = scu.hard_obs(r, T_SCALE), scu.base_weights(r, T_SCALE)
    return r, obs, base, stream_rows(r, obs, base, L, SCALE_SPLITS)


@pytest.mark.parametrize("L", [0, 5])
@pytest.mark.parametrize("name,big", GRID, ids=["%s-%d" % g for g in GRID])
def test_scale_patterns(name, big, L):
    r, obs, base, (rows0, ll0, st0) = scale_base(name, L)
    check((rows0, ll0, st0), oracle(r, obs, base, L))
    k = scu.exponents(T_SCALE, len(r.soft), big)
    rows, ll, st = stream_rows(r, obs, scu.scaled(base, k), L, SCALE_SPLITS)
    assert np.all(st == 0) and np.all(st0 == 0)
    moved = [b for b in range(scu.B) if not np.array_equal(rows[b], rows0[b])]
    assert not moved, "rows differ from the unscaled run's in sequences %s" % moved
    tg.check_ll(ll, ll0 + k.sum(axis=(1, 2)) * LN2)


@pytest.mark.parametrize("L", [0, 5])
@pytest.mark.parametrize("name", scu.NAMES)
def test_edge_batch(name, L):
    """A spread inside the vector, denormal vectors, DBL_MAX vectors."""
    r = scu.requests()[name]
    obs, liks = scu.hard_obs(r, T_SCALE), scu.edge_weights(r, T_SCALE)
    want = oracle(r, obs, liks, L)
    assert np.all(want[2] == 0)
    check(stream_rows(r, obs, liks, L, SCALE_SPLITS), want)


def test_every_vector_at_2_to_the_1000():
    """300 steps: the exponent sum is 300 000 and no value overflows."""
    r = requests()["hmm16"]
    B, T, L = 5, 300, 5
    obs, liks = inputs(r, B, T, 41)
    rows0, ll0, st0 = stream_rows(r, obs, liks, L, (100, 64, 136))
    rows, ll, st = stream_rows(r, obs, [np.ldexp(w, 1000) for w in liks], L, (100, 64, 136))
    assert np.isfinite(rows).all() and np.isfinite(ll).all() and np.all(st == 0) and np.all(st0 == 0)
    assert np.array_equal(rows, rows0)
    tg.check_ll(ll, ll0 + T * 1000 * LN2)
    assert np.all(ll > 2e5)


# ---------------------------------------------------------------------------
# 5. dead sequences and bad weights

def _dead_case():
    m, P1, M1, tables = tg.hmm(3, 4, False)
    r = scu.Req("hmm3", m, tables, (0,), (), [M1], [], [P1], None)
    return r, tg.weights(4, 12, (4,), 17)[0]


@pytest.mark.parametrize("value", [0.0, np.nan, -1.0, np.inf], ids=["zero-vector", "nan", "negative", "inf"])
def test_a_sequence_dies_at_step_6(value):
    """L = 5, pushes of 4, 4, 4 and a flush; the vector of step 6 of sequence 1
    is all zero, or holds one bad weight."""
    r, w = _dead_case()
    L, d = 5, 6
    gtrace = []
    good = stream_rows(r, None, [w], L, (4, 4, 4), trace=gtrace)
    bad = w.copy()
    if value == 0.0:
        bad[1, d] = 0.0
    else:
        bad[1, d, 2] = value
    status = 1 if value == 0.0 else BAD
    trace = []
    rows, ll, st = stream_rows(r, None, [bad], L, (4, 4, 4), trace=trace)
    assert not np.isnan(rows).any() and all(not np.isnan(t[0]).any() for t in trace)
    # row 0 (endpoint 5) comes out of the second push, alive; the rows from 1 on end at d or later
    assert np.array_equal(rows[1, 0], good[0][1, 0]) and np.all(rows[1, 1:] == 0.0)
    # ll and status after the pushes of steps 0..3, 4..7, 8..11 and the flush
    assert trace[0][0][1] == gtrace[0][0][1] and trace[0][1][1] == 0
    for ll_k, st_k in trace[1:]:
        assert ll_k[1] == -DBL_MAX and st_k[1] == status
    assert list(st) == [0, status, 0, 0]
    keep = [0, 2, 3]
    for (ll_k, st_k), (gll, gst) in zip(trace, gtrace):
        assert np.array_equal(ll_k[keep], gll[keep]) and np.array_equal(st_k[keep], gst[keep])
    assert np.array_equal(rows[keep], good[0][keep])
    want = oracle(r, None, [bad], L)
    check((rows, ll, st), want)


# ---------------------------------------------------------------------------
# 6. lifecycle

def test_lifecycle():
    r = requests()["hmm16"]
    B, T, L = 5, 20, 3
    obs, liks = inputs(r, B, T, 51)
    w = cuda(liks[0], np.float64)
    with nip_amd.Stream(r.m, r.ov, r.q, B, lag=L, soft_vars=r.sv) as s:
        first = feed(s, obs, liks, (4, 9, 7))
        with pytest.raises(nip_amd.NipError) as e:
            s.push(None, lik=w[:, :2].contiguous())                                  # after the flush
        assert e.value.code == nip_amd.NIP_ERROR_INVALID_ARGUMENT
        assert s.steps == T and s.pending == 0
        s.reset()
        assert s.steps == 0 and s.pending == 0
        again = feed(s, obs, liks, (4, 9, 7))
        same_bits(first, again)
        s.reset()
        # the hard push of the C ABI on a stream with soft columns; T < 1; a missing buffer
        lib = nip_amd.lib()
        o = torch.zeros((B, 2, 1), dtype=torch.int32, device="cuda")
        post = torch.zeros((B, 8, 16), dtype=torch.float64, device="cuda")
        ptr = lambda t: C.c_void_p(t.data_ptr())
        assert lib.nipamd_stream_push(s._h, ptr(o), 2, ptr(post), None, None, None) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
        assert lib.nipamd_stream_push_host(s._h, ptr(o), 2, ptr(post), None, None) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
        assert lib.nipamd_stream_push_soft(s._h, None, ptr(w), 0, ptr(post), None, None, None) == \
            nip_amd.NIP_ERROR_INVALID_ARGUMENT
        assert lib.nipamd_stream_push_soft(s._h, None, None, 2, ptr(post), None, None, None) == \
            nip_amd.NIP_ERROR_NULLPOINTER
        assert lib.nipamd_stream_push_soft(s._h, None, ptr(w), 8, None, None, None, None) == \
            nip_amd.NIP_ERROR_NULLPOINTER                                             # 8 steps at lag 3 emit
        assert s.steps == 0
    with pytest.raises(nip_amd.NipError):
        s.push(None, lik=w[:, :2].contiguous())                                      # closed


# ---------------------------------------------------------------------------
# 7. buffers and forms

@pytest.mark.parametrize("name", ["demo20-one-soft", "factorial-y"])
def test_guard_bands(name):
    """post is a slice of a larger tensor with 64 doubles of sentinel on either side."""
    B, L = 3, 3
    if name == "demo20-one-soft":
        m, v, _ = tg.demo1(20)
        sv, q, cards, width = [v["A1"]], [v["C1"]], (20,), 20
    else:
        m, cur, O1, _ = tg.factorial()
        sv, q, cards, width = [O1], [m.variable("Y1")], (5,), 4
    w = cuda(tg.weights(B, 11, cards, 19)[0], np.float64)
    with nip_amd.Stream(m, [], q, B, lag=L, soft_vars=sv) as s:
        for a, b, E in ((0, 2, 0), (2, 11, 8), (11, 11, 3)):
            n = B * E * width
            big = torch.full((n + 128,), -7.25, dtype=torch.float64, device="cuda")
            post = big[64:64 + n].view(B, E, width)
            got = s.push(None, post=post, lik=w[:, a:b].contiguous()) if b > a else s.flush(post=post)
            assert nip_amd.last_kernel() == KERNEL and got is post
            big = big.cpu().numpy()
            assert np.all(big[:64] == -7.25) and np.all(big[64 + n:] == -7.25)
            rows = post.cpu().numpy()
            assert np.all(rows >= 0.0) and (E == 0 or np.abs(rows.sum(axis=2) - 1.0).max() <= 1e-12)
        assert np.all(s.status.cpu().numpy() == 0)


def test_callers_buffers_and_stream():
    """Rows, ll and status in the caller's tensors (ll and status between
    sentinels), on a HIP stream of the caller's."""
    r = requests()["hmm16"]
    B, L = 13, 4
    obs, liks = inputs(r, B, 30, 61)
    want = stream_rows(r, obs, liks, L, (10, 20))
    w = cuda(liks[0], np.float64)
    hs = torch.cuda.Stream()
    hs.wait_stream(torch.cuda.current_stream())
    with nip_amd.Stream(r.m, r.ov, r.q, B, lag=L, soft_vars=r.sv) as s, torch.cuda.stream(hs):
        llbuf = torch.full((B + 16,), -7.0, dtype=torch.float64, device="cuda")
        stbuf = torch.full((B + 16,), -7, dtype=torch.int32, device="cuda")
        s.ll, s.status = llbuf[8:8 + B], stbuf[8:8 + B]
        p1 = torch.full((B, 6, 16), -7.0, dtype=torch.float64, device="cuda")
        p2 = torch.full((B, 20, 16), -7.0, dtype=torch.float64, device="cuda")
        p3 = torch.full((B, 4, 16), -7.0, dtype=torch.float64, device="cuda")
        assert s.push(None, post=p1, stream=hs, lik=w[:, :10].contiguous()) is p1
        assert s.push(None, post=p2, stream=hs, lik=w[:, 10:].contiguous()) is p2
        assert nip_amd.last_kernel() == KERNEL
        assert s.flush(post=p3, stream=hs) is p3
        hs.synchronize()
        assert np.array_equal(torch.cat([p1, p2, p3], dim=1).cpu().numpy(), want[0])
        llb, stb = llbuf.cpu().numpy(), stbuf.cpu().numpy()
        assert np.array_equal(llb[8:8 + B], want[1]) and np.array_equal(stb[8:8 + B], want[2])
        assert np.all(llb[:8] == -7.0) and np.all(llb[8 + B:] == -7.0)
        assert np.all(stb[:8] == -7) and np.all(stb[8 + B:] == -7)
        s.reset(stream=hs)
        with pytest.raises(nip_amd.NipError):
            s.push(None, lik=w[:, :10].contiguous(), post=torch.zeros((B, 6, 16), device="cuda"))   # float32
        with pytest.raises(nip_amd.NipError):
            s.push(None, lik=w[:, :10].contiguous(),
                   post=torch.zeros((B, 7, 16), dtype=torch.float64, device="cuda"))
        assert s.steps == 0


def test_python_argument_checks():
    m, P1, M1, _ = tg.hmm(3, 4, False)
    w = torch.ones((2, 3, 4), dtype=torch.float64, device="cuda")
    o = torch.zeros((2, 3, 1), dtype=torch.int32, device="cuda")
    with nip_amd.Stream(m, [], [P1], 2, lag=1, soft_vars=[M1]) as s:
        for bad in (w.float(), w[:, :, :3].contiguous(), w.cpu(), w.transpose(0, 1), w[:1].contiguous(), None):
            with pytest.raises(nip_amd.NipError) as e:
                s.push(None, lik=bad)
            assert e.value.code == nip_amd.NIP_ERROR_INVALID_ARGUMENT
        assert s.steps == 0
    with nip_amd.Stream(m, [P1], [P1], 2, lag=1, soft_vars=[M1]) as s:
        for bad in (None, o[:, :2].contiguous(), o.to(torch.int64), o.cpu()):       # missing, another T, dtype, device
            with pytest.raises(nip_amd.NipError) as e:
                s.push(bad, lik=w)
            assert e.value.code == nip_amd.NIP_ERROR_INVALID_ARGUMENT
        assert s.steps == 0
        assert tuple(s.push(o, lik=w).shape) == (2, 2, 3)
    with nip_amd.Stream(m, [M1], [P1], 2, lag=1) as s:                               # no soft columns: no lik
        with pytest.raises(nip_amd.NipError) as e:
            s.push(o, lik=w)
        assert e.value.code == nip_amd.NIP_ERROR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", ["hmm16", "demo20-a-soft-b-hard"])
def test_host_form_is_the_device_form(name):
    r = requests()[name]
    B, L = 6, 2
    obs, liks = inputs(r, B, 21, 71)
    want = stream_rows(r, obs, liks, L, (1, 8, 12))
    w = np.concatenate(liks, axis=2)
    with nip_amd.Stream(r.m, r.ov, r.q, B, lag=L, soft_vars=r.sv) as s:
        out = []
        for a, b in ((0, 1), (1, 9), (9, 21)):
            post, ll, st = s.push_host(obs[:, a:b] if r.ov else None, lik=w[:, a:b])
            assert nip_amd.last_kernel() == KERNEL
            assert post.shape == (B, max(0, min(a, L) + (b - a) - L), s.width)
            out.append(post)
        post, ll, st = s.flush_host()
        out.append(post)
        assert s.steps == 21 and s.pending == 0
    assert np.array_equal(np.concatenate(out, axis=1), want[0])
    assert np.array_equal(ll, want[1]) and np.array_equal(st.astype(np.int32), want[2])


# ---------------------------------------------------------------------------
# 8. one stream's rows are the next stream's evidence

def test_cascade():
    """Stream 1 (hard evidence, lag 3) emits rows of P1; whenever it emits, the
    tensor it returned is pushed as the likelihood vectors of Q1 of a second
    model (lag 2)."""
    m, P1, M1, _ = tg.hmm(16, 16, False)
    m2, Q1, _, (A, pi, Es) = tg.hmm(16, 16, True, seed=5)
    B, T = 5, 30
    o = cuda(tg.gappy(B, T, (16,), 91), np.int32)
    fed, out = [], []
    with nip_amd.Stream(m, [M1], [P1], B, lag=3) as s1, nip_amd.Stream(m2, [], [Q1], B, lag=2, soft_vars=[Q1]) as s2:
        pos = 0
        for n in (2, 1, 5, 9, 13, 0):                        # 0: the flush
            rows = s1.push(o[:, pos:pos + n].contiguous()) if n else s1.flush()
            pos += n
            if rows.shape[1] > 0:
                fed.append(rows)
                out.append(s2.push(None, lik=rows))
                assert nip_amd.last_kernel() == KERNEL
        out.append(s2.flush())
        torch.cuda.synchronize()
        assert s2.steps == T and len(fed) >= 3
        got = torch.cat(out, dim=1).cpu().numpy(), s2.ll.cpu().numpy(), s2.status.cpu().numpy()
    lik = torch.cat(fed, dim=1).cpu().numpy()
    assert lik.shape == (B, T, 16)
    want = ssu.soft_fixed_lag(A, pi, Es + [np.eye(16)], [so.HARD, so.SOFT], [np.full((B, T), -1), None], [None, lik], 2)
    check(got, want)
