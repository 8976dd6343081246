"""Online inference under soft evidence (nipamd_stream_open_soft,
nipamd_stream_push_soft, nipamd_stream_push_soft_host, nip_amd.Stream with
soft_vars) without a GPU: the exported symbols, the argument and scope verdicts
of nipamd_stream_open_soft (decided on the host, before anything touches the
device: the union of nipamd_stream_open's and nipamd_fb_soft's), the
NULL-handle calls, and the numpy oracle of tests/test_gpu_soft_stream.py
(soft_stream_util.soft_fixed_lag) pinned to soft_util.soft_smoother and
stream_util.fixed_lag.  The verdicts of a push on an open stream need a device
and are in tests/test_gpu_soft_stream.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nip_amd
from nip_amd import synth

import soft_stream_util as ssu
import soft_util as so
import stream_util as su
from viterbi_util import DBL_MAX

NAMES = ["nipamd_stream_open_soft", "nipamd_stream_push_soft", "nipamd_stream_push_soft_host"]
NULL, INVALID = nip_amd.NIP_ERROR_NULLPOINTER, nip_amd.NIP_ERROR_INVALID_ARGUMENT
OK = (0, nip_amd.NIPAMD_ERROR_DEVICE)


def spec_model(spec):
    nodes, pots = spec
    return nip_amd.Model.from_spec(nodes, pots)


def open_(m, obs_vars, soft_vars, query, B=2, lag=1, handle=True, out=True, ov_ptr=True, sv_ptr=True, q_ptr=True,
          n_soft=None):
    """nipamd_stream_open_soft; a stream that does open (a GPU is present) is freed again."""
    L = nip_amd.lib()
    h = C.c_void_p()
    rc = L.nipamd_stream_open_soft(m._h if handle else None, len(obs_vars),
                                   nip_amd._ints(obs_vars) if ov_ptr else None,
                                   len(soft_vars) if n_soft is None else n_soft,
                                   nip_amd._ints(soft_vars) if sv_ptr else None, len(query),
                                   nip_amd._ints(query) if q_ptr else None, B, lag, C.byref(h) if out else None)
    if rc == 0:
        L.nipamd_stream_free(h)
    return rc


def unsupported(rc):
    assert rc == nip_amd.NIPAMD_ERROR_UNSUPPORTED, rc
    msg = nip_amd.lib().nipamd_last_error().decode()
    assert msg.strip()
    return msg


def five_children():
    nodes = [("P0", 3, "P1"), ("P1", 3, None)] + [("O%d" % k, 2, None) for k in range(5)]
    pots = [("P1", ["P0"], synth.cpt(1, 3, 3)), ("P0", [], synth.cpt(2, 3, 1))]
    pots += [("O%d" % k, ["P1"], synth.cpt(3 + k, 2, 3)) for k in range(5)]
    w = nip_amd.Model.from_spec(nodes, pots)
    return w, [w.variable("O%d" % k) for k in range(5)], w.variable("P1")


def test_symbols_exported():
    L = C.CDLL(nip_amd.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nip_amd.h")).read()
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in nip_amd.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    import inspect
    assert "soft_vars" in inspect.signature(nip_amd.Stream.__init__).parameters
    assert "lik" in inspect.signature(nip_amd.Stream.push).parameters
    assert "lik" in inspect.signature(nip_amd.Stream.push_host).parameters


def test_null_handle():
    L = nip_amd.lib()
    buf = np.zeros(8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.nipamd_stream_push_soft(None, p, p, 1, p, None, None, None) == NULL
    assert L.nipamd_stream_push_soft_host(None, p, p, 1, p, None, None) == NULL
    assert nip_amd.lib().nipamd_last_error().decode().strip()


def test_argument_errors():
    m = spec_model(synth.hmm_spec(3, 4))
    P1, M1 = m.variable("P1"), m.variable("M1")
    for engine in (nip_amd.ENGINE_AUTO, nip_amd.ENGINE_JTREE):         # the arguments are decided before the scope
        m.set_engine(engine)
        assert open_(m, [], [M1], [P1], handle=False) == NULL
        assert open_(m, [], [M1], [P1], out=False) == NULL
        assert open_(m, [M1], [P1], [P1], ov_ptr=False) == NULL
        assert open_(m, [], [M1], [P1], sv_ptr=False) == NULL
        assert open_(m, [], [M1], [P1], q_ptr=False) == NULL
        for kw in (dict(B=0), dict(B=-3), dict(lag=-1), dict(lag=nip_amd.STREAM_MAX_LAG + 1), dict(n_soft=-1)):
            assert open_(m, [], [M1], [P1], **kw) == INVALID, kw
            assert nip_amd.lib().nipamd_last_error().decode().strip()
        for bad in (99, -1):
            assert open_(m, [bad], [M1], [P1]) == INVALID
            assert open_(m, [], [bad], [P1]) == INVALID
            assert open_(m, [], [M1], [bad]) == INVALID
            assert nip_amd.lib().nipamd_last_error().decode().strip()
    # a variable in both lists is a matter of scope: the bad argument beside it decides
    m.set_engine(nip_amd.ENGINE_AUTO)
    assert open_(m, [M1], [M1], [P1], B=0) == INVALID


def test_scope_refusals():
    n = spec_model(synth.nonleaf_spec())
    assert "chain" in unsupported(open_(n, [], [n.variable("Q1")], [n.variable("P1")]))
    m = spec_model(synth.hmm_spec(3, 4))
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    m.set_engine(nip_amd.ENGINE_JTREE)
    assert "JTREE" in unsupported(open_(m, [], [M1], [P1]))
    m.set_engine(nip_amd.ENGINE_AUTO)
    assert "hard and as soft" in unsupported(open_(m, [M1], [M1], [P1]))
    unsupported(open_(m, [], [M1, M1], [P1]))                          # twice in soft_vars
    unsupported(open_(m, [], [P0], [P1]))                              # neither the interface nor a leaf child
    unsupported(open_(m, [M1], [P0], [P1]))
    w, ov, wP1 = five_children()
    assert "four" in unsupported(open_(w, ov[:3], ov[3:], [wP1]))      # 3 hard + 2 soft
    assert "four" in unsupported(open_(w, [], ov, [wP1]))
    for q in ([M1], [P0], [P1, P1], [P1, M1], []):
        assert "interface" in unsupported(open_(m, [], [M1], q)), q
    f = spec_model(synth.factorial_spec(4, 4, 5))
    X0, X1, Y1, O1 = f.variable("X0"), f.variable("X1"), f.variable("Y1"), f.variable("O1")
    for q in ([O1], [X0], [X1, X1], [X1, Y1, O1], []):
        assert "interface" in unsupported(open_(f, [], [O1], q)), q
    unsupported(open_(f, [], [X0], [X1]))


def test_lds_need_beyond_a_cu():
    """64 states and four soft children of 64 states each: 4 x 66 table rows of
    512 bytes and two 32 KB images of A are more than a CU's 160 KB."""
    nodes = [("P0", 64, "P1"), ("P1", 64, None)] + [("O%d" % k, 64, None) for k in range(4)]
    pots = [("P1", ["P0"], synth.cpt(1, 64, 64)), ("P0", [], synth.cpt(2, 64, 1))]
    pots += [("O%d" % k, ["P1"], synth.cpt(3 + k, 64, 64)) for k in range(4)]
    w = nip_amd.Model.from_spec(nodes, pots)
    ov = [w.variable("O%d" % k) for k in range(4)]
    msg = unsupported(open_(w, [], ov, [w.variable("P1")], lag=4))
    assert "LDS" in msg and re.search(r"\d{6} bytes", msg), msg
    assert open_(w, [], ov[:1], [w.variable("P1")], lag=4) in OK


def test_a_request_in_scope_passes_the_host_verdict():
    """Everything in scope: the stream opens where there is a GPU, and fails
    with the device error -- not a refusal -- where there is none."""
    m = spec_model(synth.hmm_spec(3, 4))
    P1, M1 = m.variable("P1"), m.variable("M1")
    for lag in (0, 1, nip_amd.STREAM_MAX_LAG):
        assert open_(m, [], [M1], [P1], lag=lag) in OK
    assert open_(m, [], [P1], [P1]) in OK                              # the interface variable itself
    assert open_(m, [M1], [P1], [P1]) in OK                            # hard and soft columns together
    assert open_(m, [P1], [M1], [P1]) in OK
    assert open_(m, [M1], [], [P1]) in OK                              # n_soft == 0: the hard stream
    assert open_(m, [M1], [], [P1], sv_ptr=False) in OK
    assert open_(m, [], [], [P1]) in OK
    w, ov, wP1 = five_children()
    assert open_(w, ov[:2], ov[2:4], [wP1]) in OK
    assert open_(w, [], ov[:4], [wP1], lag=nip_amd.STREAM_MAX_LAG) in OK
    f = spec_model(synth.factorial_spec(4, 4, 5))
    X1, Y1, O1 = f.variable("X1"), f.variable("Y1"), f.variable("O1")
    for q in ([X1, Y1], [Y1, X1], [Y1], [X1]):
        assert open_(f, [], [O1], q, lag=3) in OK


def test_python_stream_without_soft_vars_is_the_hard_stream():
    """soft_vars=() goes through nipamd_stream_open: the verdicts are its own."""
    m = spec_model(synth.hmm_spec(3, 4))
    P1, M1 = m.variable("P1"), m.variable("M1")
    for sv in ((), [M1]):
        with pytest.raises(nip_amd.NipError) as e:
            nip_amd.Stream(m, [], [P1], 0, lag=1, soft_vars=sv)
        assert e.value.code == INVALID
    with pytest.raises(nip_amd.NipError) as e:
        nip_amd.Stream(m, [M1], [P1], 2, lag=1, soft_vars=[M1])
    assert e.value.code == nip_amd.NIPAMD_ERROR_UNSUPPORTED


# ---------------------------------------------------------------------------
# the oracle, pinned

B_, T_, M_ = 4, 12, 5
LAGS = (0, 1, 2, 5, 11, 40)


def tables(N, seed):
    rng = np.random.default_rng(seed)
    A = rng.random((N, N)) + 0.05
    A /= A.sum(axis=1, keepdims=True)
    pi = rng.random(N) + 0.05
    pi /= pi.sum()
    E = rng.random((N, M_)) + 0.05                                 # rows do not sum to 1: the ll's m1 term matters
    return rng, A, pi, E


@pytest.mark.parametrize("N", [3, 16])
def test_lag_0_is_filtering_and_a_long_lag_smoothing(N):
    rng, A, pi, E = tables(N, 80 + N)
    E2 = rng.random((N, 3)) + 0.05
    codes = rng.integers(-1, 3, size=(B_, T_))
    w = 0.05 + rng.random((B_, T_, M_))
    args = ([E, E2], [so.SOFT, so.HARD], [None, codes], [w, None])
    smoothed, filtered, ll = so.soft_smoother(A, pi, *args)
    for L in LAGS:
        rows, ll_l, st = ssu.soft_fixed_lag(A, pi, *args, L)
        assert np.array_equal(ll_l, ll) and np.all(st == 0)
        assert np.abs(rows.sum(axis=2) - 1.0).max() <= 1e-14
        if L == 0:
            assert np.abs(rows - filtered).max() <= 1e-15
        if L >= T_ - 1:
            assert np.abs(rows - smoothed).max() <= 1e-13
        # row t is row t of the smoother run on the steps up to the row's endpoint
        for t in range(T_):
            end = min(t + L, T_ - 1)
            want, _, _ = so.soft_smoother(A, pi, [E, E2], [so.SOFT, so.HARD], [None, codes[:, :end + 1]],
                                          [w[:, :end + 1], None])
            assert np.abs(rows[:, t] - want[:, t]).max() <= 1e-13, (L, t)


@pytest.mark.parametrize("N", [3, 16])
def test_one_hot_and_all_ones_weights_are_the_hard_stream(N):
    rng, A, pi, E = tables(N, 90 + N)
    codes = rng.integers(-1, M_, size=(B_, T_))                        # -1: missing
    w = np.eye(M_)[np.maximum(codes, 0)]
    w[codes < 0] = 1.0
    for L in LAGS:
        want, want_ll = su.fixed_lag(A, pi, [E], [codes], L)
        rows, ll, st = ssu.soft_fixed_lag(A, pi, [E], [so.SOFT], [None], [w], L)
        assert np.abs(rows - want).max() <= 1e-13 and np.abs(ll - want_ll).max() <= 1e-12
        assert np.all(st == 0)


@pytest.mark.parametrize("value,status", [(0.0, 1), (np.nan, 5), (-1.0, 5), (np.inf, 5)])
@pytest.mark.parametrize("N", [3, 16])
def test_dead_sequences_follow_the_streams_rule(N, value, status):
    rng, A, pi, E = tables(N, 100 + N)
    w = 0.05 + rng.random((B_, T_, M_))
    d = 6
    bad = w.copy()
    if value == 0.0:
        bad[1, d] = 0.0
    else:
        bad[1, d, 2] = value
    for L in LAGS:
        good = ssu.soft_fixed_lag(A, pi, [E], [so.SOFT], [None], [w], L)
        rows, ll, st = ssu.soft_fixed_lag(A, pi, [E], [so.SOFT], [None], [bad], L)
        assert list(st) == [0, status, 0, 0] and ll[1] == -DBL_MAX
        assert not np.isnan(rows).any() and not np.isnan(ll).any()
        for t in range(T_):
            if min(t + L, T_ - 1) >= d:
                assert np.all(rows[1, t] == 0.0), (L, t)
            else:
                assert np.array_equal(rows[1, t], good[0][1, t]), (L, t)
        keep = [0, 2, 3]
        assert np.array_equal(rows[keep], good[0][keep]) and np.array_equal(ll[keep], good[1][keep])
