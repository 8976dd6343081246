"""mlss / most_likely_states without a GPU: the exported symbols, the argument
and scope verdicts of nipamd_mlss / nipamd_mlss_host (decided on the host,
before anything touches the device), and the numpy oracle of
tests/test_gpu_viterbi.py against its own brute force."""
import ctypes as C

import numpy as np
import pytest

import nip_amd
from nip_amd import build, synth

import viterbi_util as vu


def spec_model(spec):
    nodes, pots = spec
    return nip_amd.Model.from_spec(nodes, pots)


def call(m, obs_vars, query, B=2, T=3, host=False, obs=True, path=True, handle=True):
    """nipamd_mlss / _host with real (host) buffers behind every pointer: the
    calls below are all refused before a buffer is followed."""
    L = nip_amd.lib()
    o = np.zeros((max(B, 1), max(T, 1), max(len(obs_vars), 1)), np.int32)
    p = np.zeros((max(B, 1), max(T, 1), max(len(query), 1)), np.int32)
    lp = np.zeros(max(B, 1))
    st = np.zeros(max(B, 1), np.uint32)
    args = [m._h if handle else None, o.ctypes.data_as(C.c_void_p) if obs else None, len(obs_vars),
            nip_amd._ints(obs_vars), B, T, len(query), nip_amd._ints(query),
            p.ctypes.data_as(C.c_void_p) if path else None, lp.ctypes.data_as(C.c_void_p),
            st.ctypes.data_as(C.c_void_p)]
    if host:
        return L.nipamd_mlss_host(*args)
    return L.nipamd_mlss(*args, None)


def test_symbols_exported():
    L = C.CDLL(nip_amd.LIB_PATH)
    assert hasattr(L, "nipamd_mlss") and hasattr(L, "nipamd_mlss_host")
    nip_amd.lib()
    assert hasattr(C.CDLL(build.COMPAT_LIB), "mlss")
    assert callable(nip_amd.most_likely_states) and callable(nip_amd.most_likely_states_host)


@pytest.mark.parametrize("host", [False, True])
def test_argument_errors(host):
    m = spec_model(synth.hmm_spec(3, 4))
    P1, M1 = m.variable("P1"), m.variable("M1")
    assert call(m, [M1], [P1], host=host, handle=False) == nip_amd.NIP_ERROR_NULLPOINTER
    assert call(m, [M1], [P1], host=host, obs=False) == nip_amd.NIP_ERROR_NULLPOINTER
    assert call(m, [M1], [P1], host=host, path=False) == nip_amd.NIP_ERROR_NULLPOINTER
    assert call(m, [M1], [P1], host=host, B=0) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert call(m, [M1], [P1], host=host, B=-1) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert call(m, [M1], [P1], host=host, T=0) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert call(m, [M1], [P1], host=host, T=-5) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert call(m, [M1], [99], host=host) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert call(m, [M1], [-1], host=host) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert call(m, [99], [P1], host=host) == nip_amd.NIP_ERROR_INVALID_ARGUMENT


def unsupported(rc):
    assert rc == nip_amd.NIPAMD_ERROR_UNSUPPORTED, rc
    msg = nip_amd.lib().nipamd_last_error().decode()
    assert msg.strip()
    return msg


@pytest.mark.parametrize("host", [False, True])
def test_query_must_be_the_interface(host):
    m = spec_model(synth.hmm_spec(3, 4))
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    assert "interface" in unsupported(call(m, [M1], [M1], host=host))
    unsupported(call(m, [M1], [P0], host=host))
    unsupported(call(m, [M1], [P1, M1], host=host))
    unsupported(call(m, [M1], [P1, P1], host=host))
    unsupported(call(m, [M1], [], host=host))
    f = spec_model(synth.factorial_spec(4, 4, 5))
    X1, Y1, O1 = f.variable("X1"), f.variable("Y1"), f.variable("O1")
    assert "interface" in unsupported(call(f, [O1], [X1], host=host))
    unsupported(call(f, [O1], [X1, X1], host=host))
    unsupported(call(f, [O1], [X1, Y1, O1], host=host))


@pytest.mark.parametrize("host", [False, True])
def test_evidence_the_plan_does_not_route(host):
    m = spec_model(synth.hmm_spec(3, 4))
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    unsupported(call(m, [P0], [P1], host=host))                  # neither the interface nor a leaf child
    unsupported(call(m, [M1, M1], [P1], host=host))              # listed twice
    # more than four observed columns: five leaf children, all observed
    nodes = [("P0", 3, "P1"), ("P1", 3, None)] + [("O%d" % k, 2, None) for k in range(5)]
    pots = [("P1", ["P0"], synth.cpt(1, 3, 3)), ("P0", [], synth.cpt(2, 3, 1))]
    pots += [("O%d" % k, ["P1"], synth.cpt(3 + k, 2, 3)) for k in range(5)]
    w = nip_amd.Model.from_spec(nodes, pots)
    ov = [w.variable("O%d" % k) for k in range(5)]
    assert "four" in unsupported(call(w, ov, [w.variable("P1")], host=host))


@pytest.mark.parametrize("host", [False, True])
def test_no_chain_plan_or_general_engine(host):
    n = spec_model(synth.nonleaf_spec())
    msg = unsupported(call(n, [n.variable("Q1")], [n.variable("P1")], host=host))
    assert "chain" in msg
    m = spec_model(synth.hmm_spec(3, 4))
    m.set_engine(nip_amd.ENGINE_JTREE)
    msg = unsupported(call(m, [m.variable("M1")], [m.variable("P1")], host=host))
    assert "JTREE" in msg


def test_oracle_against_its_brute_force():
    """viterbi_util.viterbi on 3 states, T = 6: its logp is the maximum of
    path_score over all 729 paths, its path attains it and (no ties in random
    tables) is the maximiser."""
    rng = np.random.default_rng(3)
    A = rng.random((3, 3))
    pi = rng.random(3)
    E = rng.random((3, 4))
    cols = [rng.integers(-1, 4, size=(8, 6))]
    path, logp = vu.viterbi(A, pi, [E], cols)
    score = vu.path_score(A, pi, [E], cols, path)
    for b in range(8):
        best, arg = vu.brute_force(A, pi, [E], [cols[0][b]])
        assert abs(logp[b] - best) <= 1e-13 * max(1.0, abs(best))
        assert abs(score[b] - best) <= 1e-13 * max(1.0, abs(best))
        assert np.array_equal(path[b], arg)


def test_oracle_ties_zero_mass_and_scaling():
    """Exact ties resolve to the lowest state; an out-of-range code leaves no
    mass; 3000 steps neither underflow nor lose the optimum."""
    A = np.full((4, 4), 0.25)
    pi = np.full(4, 0.25)
    E = np.full((4, 2), 0.5)
    cols = [np.zeros((2, 5), np.int64)]
    cols[0][1, 3] = 2
    path, logp = vu.viterbi(A, pi, [E], cols)
    assert np.array_equal(path[0], np.zeros(5)) and np.array_equal(path[1], -np.ones(5))
    assert abs(logp[0] + 15 * np.log(2.0)) <= 1e-13          # u0 = 2^-2, five e = 2^-1, four A = 2^-2
    assert logp[1] == -vu.DBL_MAX
    rng = np.random.default_rng(5)
    A = rng.random((5, 5)); A /= A.sum(axis=1, keepdims=True)
    pi = rng.random(5); pi /= pi.sum()
    E = rng.random((5, 6)); E /= E.sum(axis=1, keepdims=True)
    cols = [rng.integers(0, 6, size=(2, 3000))]
    path, logp = vu.viterbi(A, pi, [E], cols)
    assert np.all(np.isfinite(logp)) and np.all(logp < -3000)
    score = vu.path_score(A, pi, [E], cols, path)
    assert np.all(np.abs(score - logp) <= 1e-11 * np.abs(logp))
