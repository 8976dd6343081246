"""Online inference (nipamd_stream_*, nip_amd.Stream) without a GPU: the
exported symbols, the argument and scope verdicts of nipamd_stream_open
(decided on the host, before anything touches the device), the NULL-handle
accessors, and the numpy oracle of tests/test_gpu_stream.py
(stream_util.fixed_lag) pinned to textbook_util.smoother run on each prefix."""
import ctypes as C

import numpy as np
import pytest

import nip_amd
from nip_amd import synth

import stream_util as su
from textbook_util import smoother


def spec_model(spec):
    nodes, pots = spec
    return nip_amd.Model.from_spec(nodes, pots)


def open_(m, obs_vars, query, B=2, lag=1, handle=True, out=True, ov_ptr=True, q_ptr=True):
    """nipamd_stream_open; a stream that does open (a GPU is present) is freed again."""
    L = nip_amd.lib()
    h = C.c_void_p()
    rc = L.nipamd_stream_open(m._h if handle else None, len(obs_vars),
                              nip_amd._ints(obs_vars) if ov_ptr else None, len(query),
                              nip_amd._ints(query) if q_ptr else None, B, lag, C.byref(h) if out else None)
    if rc == 0:
        L.nipamd_stream_free(h)
    return rc


def unsupported(rc):
    assert rc == nip_amd.NIPAMD_ERROR_UNSUPPORTED, rc
    msg = nip_amd.lib().nipamd_last_error().decode()
    assert msg.strip()
    return msg


def test_symbols_exported():
    L = C.CDLL(nip_amd.LIB_PATH)
    names = ["nipamd_stream_open", "nipamd_stream_push", "nipamd_stream_flush", "nipamd_stream_reset",
             "nipamd_stream_pending", "nipamd_stream_steps", "nipamd_stream_free",
             "nipamd_stream_push_host", "nipamd_stream_flush_host"]
    for s in names:
        assert hasattr(L, s), s
        assert s in nip_amd.EXPORTS
    assert callable(nip_amd.Stream)
    assert nip_amd.STREAM_MAX_LAG == 64 and nip_amd.STREAM_CHUNK >= 1
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nip_amd.h")).read()
    assert int(re.search(r"#define\s+NIPAMD_STREAM_MAX_LAG\s+(\d+)", hdr).group(1)) == nip_amd.STREAM_MAX_LAG
    assert int(re.search(r"#define\s+NIPAMD_STREAM_CHUNK\s+(\d+)", hdr).group(1)) == nip_amd.STREAM_CHUNK


def test_null_handle():
    L = nip_amd.lib()
    assert L.nipamd_stream_pending(None) == -1
    assert L.nipamd_stream_steps(None) == -1
    L.nipamd_stream_free(None)
    buf = np.zeros(8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.nipamd_stream_push(None, p, 1, p, None, None, None) == nip_amd.NIP_ERROR_NULLPOINTER
    assert L.nipamd_stream_flush(None, p, None, None, None) == nip_amd.NIP_ERROR_NULLPOINTER
    assert L.nipamd_stream_reset(None, None) == nip_amd.NIP_ERROR_NULLPOINTER
    assert L.nipamd_stream_push_host(None, p, 1, p, None, None) == nip_amd.NIP_ERROR_NULLPOINTER
    assert L.nipamd_stream_flush_host(None, p, None, None) == nip_amd.NIP_ERROR_NULLPOINTER


def test_argument_errors():
    m = spec_model(synth.hmm_spec(3, 4))
    P1, M1 = m.variable("P1"), m.variable("M1")
    assert open_(m, [M1], [P1], handle=False) == nip_amd.NIP_ERROR_NULLPOINTER
    assert open_(m, [M1], [P1], out=False) == nip_amd.NIP_ERROR_NULLPOINTER
    assert open_(m, [M1], [P1], ov_ptr=False) == nip_amd.NIP_ERROR_NULLPOINTER
    assert open_(m, [M1], [P1], q_ptr=False) == nip_amd.NIP_ERROR_NULLPOINTER
    assert open_(m, [M1], [P1], B=0) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert open_(m, [M1], [P1], B=-3) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert open_(m, [M1], [P1], lag=-1) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert open_(m, [M1], [P1], lag=nip_amd.STREAM_MAX_LAG + 1) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert open_(m, [M1], [99]) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert open_(m, [M1], [-1]) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert open_(m, [99], [P1]) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert open_(m, [-2], [P1]) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    # the arguments are decided before the scope
    m.set_engine(nip_amd.ENGINE_JTREE)
    assert open_(m, [M1], [P1], B=0) == nip_amd.NIP_ERROR_INVALID_ARGUMENT


def test_a_request_in_scope_passes_the_host_verdict():
    """Everything in scope: the stream opens where there is a GPU, and fails
    with the device error -- not a refusal -- where there is none."""
    m = spec_model(synth.hmm_spec(3, 4))
    P1, M1 = m.variable("P1"), m.variable("M1")
    for lag in (0, 1, nip_amd.STREAM_MAX_LAG):
        assert open_(m, [M1], [P1], lag=lag) in (0, nip_amd.NIPAMD_ERROR_DEVICE)
    assert open_(m, [], [P1]) in (0, nip_amd.NIPAMD_ERROR_DEVICE)
    assert open_(m, [M1, P1], [P1]) in (0, nip_amd.NIPAMD_ERROR_DEVICE)
    f = spec_model(synth.factorial_spec(4, 4, 5))
    X1, Y1, O1 = f.variable("X1"), f.variable("Y1"), f.variable("O1")
    for q in ([X1, Y1], [Y1, X1], [Y1], [X1]):
        assert open_(f, [O1], q) in (0, nip_amd.NIPAMD_ERROR_DEVICE)


def test_engine_and_plan_refusals():
    n = spec_model(synth.nonleaf_spec())
    assert "chain" in unsupported(open_(n, [n.variable("Q1")], [n.variable("P1")]))
    m = spec_model(synth.hmm_spec(3, 4))
    m.set_engine(nip_amd.ENGINE_JTREE)
    assert "JTREE" in unsupported(open_(m, [m.variable("M1")], [m.variable("P1")]))
    f = spec_model(synth.factorial_spec(4, 4, 5))
    f.set_engine(nip_amd.ENGINE_JTREE)
    assert "JTREE" in unsupported(open_(f, [f.variable("O1")], [f.variable("X1")]))


def test_evidence_the_plan_does_not_route():
    m = spec_model(synth.hmm_spec(3, 4))
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    unsupported(open_(m, [P0], [P1]))                            # neither the interface nor a leaf child
    unsupported(open_(m, [M1, M1], [P1]))                        # listed twice
    nodes = [("P0", 3, "P1"), ("P1", 3, None)] + [("O%d" % k, 2, None) for k in range(5)]
    pots = [("P1", ["P0"], synth.cpt(1, 3, 3)), ("P0", [], synth.cpt(2, 3, 1))]
    pots += [("O%d" % k, ["P1"], synth.cpt(3 + k, 2, 3)) for k in range(5)]
    w = nip_amd.Model.from_spec(nodes, pots)
    ov = [w.variable("O%d" % k) for k in range(5)]
    assert "four" in unsupported(open_(w, ov, [w.variable("P1")]))
    f = spec_model(synth.factorial_spec(4, 4, 5))
    unsupported(open_(f, [f.variable("X0")], [f.variable("X1")]))


def test_query_must_be_interface_variables():
    m = spec_model(synth.hmm_spec(3, 4))
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    assert "interface" in unsupported(open_(m, [M1], [M1]))
    assert "interface" in unsupported(open_(m, [M1], [P0]))
    assert "interface" in unsupported(open_(m, [M1], [P1, M1]))
    assert "interface" in unsupported(open_(m, [M1], [P1, P1]))
    assert "interface" in unsupported(open_(m, [M1], []))
    f = spec_model(synth.factorial_spec(4, 4, 5))
    X0, X1, Y1, O1 = f.variable("X0"), f.variable("X1"), f.variable("Y1"), f.variable("O1")
    assert "interface" in unsupported(open_(f, [O1], [O1]))
    assert "interface" in unsupported(open_(f, [O1], [X0]))
    assert "interface" in unsupported(open_(f, [O1], [X1, X1]))
    assert "interface" in unsupported(open_(f, [O1], [X1, Y1, O1]))
    assert "interface" in unsupported(open_(f, [O1], []))


def test_lds_need_beyond_a_cu():
    """64 states and four observed children of 64 states each: 4 x 66 table
    rows of 512 bytes and two 32 KB images of A are more than a CU's 160 KB."""
    nodes = [("P0", 64, "P1"), ("P1", 64, None)] + [("O%d" % k, 64, None) for k in range(4)]
    pots = [("P1", ["P0"], synth.cpt(1, 64, 64)), ("P0", [], synth.cpt(2, 64, 1))]
    pots += [("O%d" % k, ["P1"], synth.cpt(3 + k, 64, 64)) for k in range(4)]
    w = nip_amd.Model.from_spec(nodes, pots)
    ov = [w.variable("O%d" % k) for k in range(4)]
    assert "LDS" in unsupported(open_(w, ov, [w.variable("P1")], lag=4))
    assert open_(w, ov[:1], [w.variable("P1")], lag=4) in (0, nip_amd.NIPAMD_ERROR_DEVICE)


@pytest.mark.parametrize("N", [3, 16])
def test_fixed_lag_against_the_smoother_on_each_prefix(N):
    """Row t of fixed_lag(L) is row t of the full smoother run on steps
    0 .. min(t + L, T - 1); L = 0 gives the filtered rows, L >= T - 1 the
    smoothed ones.  1e-13: both are the same recursions, normalised alike."""
    rng = np.random.default_rng(40 + N)
    B, T, M = 4, 12, 5
    A = rng.random((N, N)) + 0.05
    A /= A.sum(axis=1, keepdims=True)
    pi = rng.random(N) + 0.05
    pi /= pi.sum()
    E = rng.random((N, M)) + 0.05                                # rows do not sum to 1: the ll's m1 term matters
    cols = [rng.integers(-1, M, size=(B, T))]
    post, ah, ll = smoother(A, pi, [E], cols)
    for L in (0, 1, 2, 5, 11, 40):
        rows, ll_l = su.fixed_lag(A, pi, [E], cols, L)
        assert np.array_equal(ll_l, ll)
        assert np.abs(rows.sum(axis=2) - 1.0).max() <= 1e-14
        for t in range(T):
            end = min(t + L, T - 1)
            want, _, _ = smoother(A, pi, [E], [cols[0][:, :end + 1]])
            assert np.abs(rows[:, t] - want[:, t]).max() <= 1e-13, (L, t)
        if L == 0:
            assert np.abs(rows - ah).max() <= 1e-15
        if L >= T - 1:
            assert np.abs(rows - post).max() <= 1e-13


def test_digit_sums_and_sticky_tables():
    rows = np.arange(12, dtype=np.float64).reshape(1, 12)
    assert np.array_equal(su.digit_sums(rows, 1, 4), [[0 + 4 + 8, 1 + 5 + 9, 2 + 6 + 10, 3 + 7 + 11]])
    assert np.array_equal(su.digit_sums(rows, 4, 3), [[0 + 1 + 2 + 3, 4 + 5 + 6 + 7, 8 + 9 + 10 + 11]])
    A, pi, E = su.sticky_tables(16, 16, 3)
    assert np.abs(A.sum(axis=1) - 1).max() <= 1e-15 and np.abs(E.sum(axis=1) - 1).max() <= 1e-15
    assert np.diag(A).min() >= 0.97
    # the compiled model's tables are the ones written (child-first declaration order)
    from textbook_util import chain_tables
    m = spec_model(su.sticky_spec(16, 16, 3))
    A2, pi2, Es2 = chain_tables(m, m.variable("P0"), m.variable("P1"), [m.variable("M1")])
    assert np.abs(A2 - A).max() <= 1e-15 and np.abs(pi2 - pi).max() <= 1e-15 and np.abs(Es2[0] - E).max() <= 1e-15
