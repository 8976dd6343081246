"""most_likely_states_soft / nipamd_mlss_soft without a GPU: the exported
symbols, the argument and scope verdicts of both entry points (decided on the
host, before anything touches the device, in the order the header gives), the
numpy oracle of tests/test_gpu_viterbi_soft.py (viterbi_soft_util) pinned to
its brute force and to viterbi_util, and the condition under which that file
caps the paths that may differ from the oracle's: on every input it compares
with the oracle, the fp64 and the long double recursion disagree on at most
2 % of a batch's sequences."""
import ctypes as C

import numpy as np
import pytest

import nip_amd
from nip_amd import synth

import soft_scale_util as ssu
import soft_util as so
import viterbi_soft_util as vsu
import viterbi_util as vu
from test_soft_api import five_children, spec_model, unsupported
from textbook_util import smoother

NAMES = ["nipamd_mlss_soft", "nipamd_mlss_soft_host"]
OK = (0, nip_amd.NIPAMD_ERROR_DEVICE)


def call(name, m, obs_vars, soft_vars, query, B=2, T=3, handle=True, obs=True, lik=True, ov_ptr=True, sv_ptr=True,
         q_ptr=True, path=True):
    """One of the two entry points on host buffers of the right size (the
    device form only tests them for NULL before it refuses or fails: every case
    here ends before a kernel could read them, there being no GPU, or runs on a
    GPU's host form)."""
    L = nip_amd.lib()
    card = lambda v: max(m.card(v), 1) if 0 <= v < m.num_vars else 1
    o = np.zeros((max(B, 1), max(T, 1), max(len(obs_vars), 1)), np.int32)
    w = np.ones((max(B, 1), max(T, 1), max(sum(card(v) for v in soft_vars), 1)))
    p = np.zeros((max(B, 1), max(T, 1), max(len(query), 1)), np.int32)
    lp, st = np.zeros(max(B, 1)), np.zeros(max(B, 1), np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [m._h if handle else None, ptr(o) if obs else None, len(obs_vars), nip_amd._ints(obs_vars) if ov_ptr else None,
            ptr(w) if lik else None, len(soft_vars), nip_amd._ints(soft_vars) if sv_ptr else None, B, T, len(query),
            nip_amd._ints(query) if q_ptr else None, ptr(p) if path else None, ptr(lp), ptr(st)]
    if not name.endswith("_host"):
        args.append(None)
    return getattr(L, name)(*args)


def star64(card, n=4):
    """64 states and n leaf children of `card` states each."""
    nodes = [("P0", 64, "P1"), ("P1", 64, None)] + [("O%d" % k, card, None) for k in range(n)]
    pots = [("P1", ["P0"], synth.cpt(1, 64, 64)), ("P0", [], synth.cpt(2, 64, 1))]
    pots += [("O%d" % k, ["P1"], synth.cpt(3 + k, card, 64)) for k in range(n)]
    w = nip_amd.Model.from_spec(nodes, pots)
    return w, [w.variable("O%d" % k) for k in range(n)], w.variable("P1")


def test_symbols_exported():
    L = C.CDLL(nip_amd.LIB_PATH)
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in nip_amd.EXPORTS
    for f in ("most_likely_states_soft", "most_likely_states_soft_host"):
        assert callable(getattr(nip_amd, f)) and f in nip_amd.__all__


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors(name):
    m = spec_model(synth.hmm_spec(3, 4))
    P1, M1 = m.variable("P1"), m.variable("M1")
    NULL, INVALID = nip_amd.NIP_ERROR_NULLPOINTER, nip_amd.NIP_ERROR_INVALID_ARGUMENT
    for engine in (nip_amd.ENGINE_AUTO, nip_amd.ENGINE_JTREE):         # the arguments are decided before the scope
        m.set_engine(engine)
        assert call(name, m, [], [M1], [P1], handle=False) == NULL
        assert call(name, m, [M1], [], [P1], ov_ptr=False) == NULL
        assert call(name, m, [], [M1], [P1], sv_ptr=False) == NULL
        assert call(name, m, [], [M1], [P1], q_ptr=False) == NULL
        assert call(name, m, [], [M1], [P1], lik=False) == NULL
        assert call(name, m, [M1], [], [P1], obs=False) == NULL
        assert call(name, m, [], [M1], [P1], path=False) == NULL
        assert call(name, m, [], [M1], [P1], B=0) == INVALID
        assert call(name, m, [], [M1], [P1], T=0) == INVALID
        assert call(name, m, [], [M1], [P1], B=-3) == INVALID
        for bad in (99, -1):
            assert call(name, m, [bad], [M1], [P1]) == INVALID
            assert call(name, m, [], [bad], [P1]) == INVALID
            assert call(name, m, [], [M1], [bad]) == INVALID


@pytest.mark.parametrize("name", NAMES)
def test_scope_refusals(name):
    n = spec_model(synth.nonleaf_spec())
    assert "chain" in unsupported(call(name, n, [], [n.variable("Q1")], [n.variable("P1")]))
    m = spec_model(synth.hmm_spec(3, 4))
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    m.set_engine(nip_amd.ENGINE_JTREE)
    assert "JTREE" in unsupported(call(name, m, [], [M1], [P1]))
    m.set_engine(nip_amd.ENGINE_AUTO)
    assert "hard and as soft" in unsupported(call(name, m, [M1], [M1], [P1]))   # in both lists
    assert "twice" in unsupported(call(name, m, [], [M1, M1], [P1]))   # twice in soft_vars
    assert "twice" in unsupported(call(name, m, [M1, M1], [], [P1]))   # twice in obs_vars
    unsupported(call(name, m, [], [P0], [P1]))                         # neither the interface nor a leaf child
    w, ov, wP1 = five_children()
    assert "four" in unsupported(call(name, w, ov[:3], ov[3:], [wP1]))  # 3 hard + 2 soft
    for q in ([M1], [P0], [P1, P1], []):
        assert "interface" in unsupported(call(name, m, [], [M1], q)), q
    # mlss's query rule, not the rows': a joint interface is queried whole
    f = spec_model(synth.factorial_spec(4, 4, 5))
    X1, Y1, O1 = f.variable("X1"), f.variable("Y1"), f.variable("O1")
    for q in ([Y1], [X1, X1], [X1, Y1, O1]):
        assert "exactly the interface" in unsupported(call(name, f, [], [O1], q)), q


@pytest.mark.parametrize("name", NAMES)
def test_the_verdicts_come_in_order(name):
    """A request wrong in several ways gets the earliest verdict: the soft
    variables' indices before the scope, the scope before the columns, a
    variable both hard and soft before the route, the route before the query."""
    m = spec_model(synth.hmm_spec(3, 4))
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    m.set_engine(nip_amd.ENGINE_JTREE)
    assert call(name, m, [], [99], [M1]) == nip_amd.NIP_ERROR_INVALID_ARGUMENT
    assert "JTREE" in unsupported(call(name, m, [M1], [M1], [M1]))
    m.set_engine(nip_amd.ENGINE_AUTO)
    assert "hard and as soft" in unsupported(call(name, m, [M1, P0], [M1], [M1]))
    assert "neither" in unsupported(call(name, m, [], [P0], [M1]))
    assert "interface" in unsupported(call(name, m, [], [M1], [M1]))


@pytest.mark.parametrize("name", NAMES)
def test_lds_need_beyond_a_cu(name):
    """The kernel stages the evidence tables, ebase and two 64-double rows for
    each of its 4 waves, and no image of A.  64 states (512-byte rows) and
    four soft children of 80 states each: evid_rows = 1 + 4 x (80 + 2) = 329
    rows, 329 x 512 + 2 x 4 x 64 x 8 = 168448 + 4096 = 172544 bytes, more than
    a CU's 163840.  With four 64-state children the need is (1 + 4 x 66) x 512
    + 4096 = 139776 bytes and the request is in scope -- where nipamd_fb_soft,
    which adds two 32 KB images of A, refuses."""
    w, ov, P1 = star64(80)
    need = (1 + 4 * (80 + 2)) * 64 * 8 + 2 * 4 * 64 * 8
    assert need == 172544 and need > 160 * 1024
    msg = unsupported(call(name, w, [], ov, [P1], B=1, T=1))
    assert "LDS" in msg and str(need) in msg
    if name.endswith("_host"):                                         # (host buffers: no device form in scope)
        assert call(name, w, [], ov[:1], [P1], B=1, T=1) in OK
        v, ov, P1 = star64(64)
        assert (1 + 4 * 66) * 512 + 4096 == 139776
        assert call(name, v, [], ov, [P1], B=1, T=1) in OK
        assert "LDS" in unsupported(call("nipamd_fb_soft_host", v, [], ov, [P1], B=1, T=1))
        assert call(name, v, [], ov[:1], [P1], B=1, T=1) in OK           # 64 states, one 64-state soft child


def test_a_request_in_scope_passes_the_host_verdict():
    """Everything in scope: the call runs where there is a GPU, and fails with
    the device error -- not a refusal -- where there is none.  (The host form:
    its buffers are real whichever it is.)"""
    name = "nipamd_mlss_soft_host"
    m = spec_model(synth.hmm_spec(3, 4))
    P1, M1 = m.variable("P1"), m.variable("M1")
    assert call(name, m, [], [M1], [P1]) in OK
    assert call(name, m, [], [P1], [P1]) in OK                         # the interface variable itself
    assert call(name, m, [M1], [P1], [P1]) in OK
    assert call(name, m, [], [], [P1]) in OK
    w, ov, wP1 = five_children()
    assert call(name, w, ov[:2], ov[2:4], [wP1]) in OK
    f = spec_model(synth.factorial_spec(4, 4, 5))
    X1, Y1, O1 = f.variable("X1"), f.variable("Y1"), f.variable("O1")
    for q in ([X1, Y1], [Y1, X1]):
        assert call(name, f, [], [O1], q) in OK


# ---------------------------------------------------------------------------
# the oracle, pinned on N = 3, M = 4, T = 6, B = 8

N_, M_, B_, T_ = vsu.BRUTE


def small(seed=3):
    rng = np.random.default_rng(seed)
    return rng, rng.random((N_, N_)), rng.random(N_), rng.random((N_, M_))


def soft1(A, pi, E, w):
    return vsu.viterbi_soft(A, pi, [E], [so.SOFT], [None], [w])


def test_oracle_against_its_brute_force():
    """logp is the maximum of path_score_soft -- the weights as given -- over
    all 729 paths; the path attains it and (no ties in random tables) is the
    maximiser."""
    rng, A, pi, E = small()
    w = np.ldexp(0.05 + rng.random((B_, T_, M_)), rng.integers(-40, 41, size=(B_, T_, 1)))
    path, logp, st = soft1(A, pi, E, w)
    assert np.all(st == 0)
    score = vsu.path_score_soft(A, pi, [E], [so.SOFT], [None], [w], path)
    for b in range(B_):
        best, arg = vsu.brute_force_soft(A, pi, [E], [so.SOFT], [None], [w], b)
        assert abs(logp[b] - best) <= 1e-13 * max(1.0, abs(best))
        assert abs(score[b] - best) <= 1e-13 * max(1.0, abs(best))
        assert np.array_equal(path[b], arg)


def test_oracle_one_hot_is_hard_and_all_ones_is_missing():
    rng, A, pi, E = small(4)
    codes = rng.integers(0, M_, size=(B_, T_))
    want, want_lp = vu.viterbi(A, pi, [E], [codes])
    path, logp, st = soft1(A, pi, E, np.eye(M_)[codes])
    assert np.array_equal(path, want) and np.all(st == 0)
    assert np.all(np.abs(logp - want_lp) <= 1e-13 * np.maximum(1.0, np.abs(want_lp)))
    # all ones: the column is missing, beside a hard column on its own table
    E2 = rng.random((N_, 3))
    c2 = rng.integers(-1, 3, size=(B_, T_))
    want, want_lp = vu.viterbi(A, pi, [E, E2], [np.full((B_, T_), -1), c2])
    path, logp, st = vsu.viterbi_soft(A, pi, [E, E2], [so.SOFT, so.HARD], [None, c2], [np.ones((B_, T_, M_)), None])
    assert np.array_equal(path, want) and np.all(st == 0)
    assert np.all(np.abs(logp - want_lp) <= 1e-13 * np.maximum(1.0, np.abs(want_lp)))


def test_oracle_scaling_a_step_moves_only_logp():
    rng, A, pi, E = small(5)
    w = 0.05 + rng.random((B_, T_, M_))
    k = rng.integers(-1000, 900, size=(B_, T_))
    path, logp, st = soft1(A, pi, E, w)
    path2, logp2, st2 = soft1(A, pi, E, np.ldexp(w, k[:, :, None]))
    assert np.array_equal(path2, path) and np.array_equal(st2, st)
    shift = k.sum(axis=1) * vu.LN2
    assert np.all(np.abs(logp2 - logp - shift) <= 1e-13 * np.maximum(1.0, np.abs(logp2)))


def test_oracle_dead_sequences_and_bad_weights():
    rng, A, pi, E = small(6)
    w = 0.05 + rng.random((B_, T_, M_))
    good = soft1(A, pi, E, w)
    assert np.all(good[2] == 0)
    for value, status in ((0.0, 1), (np.nan, 5), (-1.0, 5), (np.inf, 5)):
        wb = w.copy()
        if value == 0.0:
            wb[1, 4] = 0.0
        else:
            wb[1, 4, 2] = value
        path, logp, st = soft1(A, pi, E, wb)
        assert list(st) == [0, status] + [0] * (B_ - 2)
        assert np.all(path[1] == -1) and logp[1] == -vu.DBL_MAX and not np.isnan(logp).any()
        assert vsu.path_score_soft(A, pi, [E], [so.SOFT], [None], [wb], good[0])[1] == -np.inf
        keep = [b for b in range(B_) if b != 1]
        assert np.array_equal(path[keep], good[0][keep]) and np.array_equal(logp[keep], good[1][keep])


# ---------------------------------------------------------------------------
# the near-tie cap's condition

# (Where long double is no wider than double the two recursions are one and
# the condition holds trivially; the x87 format has 64 mantissa bits.)

def near_ties(label, case):
    """The fp64 and the long double recursion on one input: at most 2 % of the
    batch's sequences differ in path (for B = 7: none)."""
    r, obs, liks = case
    p64, lp64, st64 = vsu.oracle(r, obs, liks)
    pw, lpw, stw = vsu.oracle(r, obs, liks, dtype=np.longdouble)
    assert np.all(st64 == 0) and np.all(stw == 0), label
    B = p64.shape[0]
    differ = int((p64 != pw).any(axis=1).sum())
    print("%s: %d / %d paths differ between the fp64 and the long double oracle" % (label, differ, B))
    assert differ <= 0.02 * B, (label, differ, B)
    assert np.all(np.abs(lp64 - lpw) <= 1e-13 * np.maximum(1.0, np.abs(lpw))), label


def test_near_ties_on_every_input_the_gpu_tests_compare():
    n = 0
    for label, case in vsu.oracle_cases():
        near_ties(label, case)
        n += 1
    assert n == 4 * len(ssu.NAMES) + len(vsu.PERIODS) + 1


def test_near_ties_on_fed_back_rows():
    """The rows the GPU test feeds back come from the device; here the textbook
    smoother's, which they equal to 1e-12."""
    (m1, ov1, q1, (A, pi, Es), codes1), r2, obs2 = vsu.fed_case()
    fed = smoother(A, pi, Es, [codes1[:, :, 0]])[0]
    near_ties("fed-back rows", (r2, obs2, [fed]))
