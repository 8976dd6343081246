"""The e_step under soft evidence (nipamd_estep_soft_partial, nipamd_estep_soft,
nipamd_estep_soft_host) without a GPU: the exported symbols, the argument and
scope verdicts (decided on the host, before anything touches the device), the
Python wrappers' input checks, and the numpy oracle of
tests/test_gpu_estep_soft.py (estep_soft_util.soft_sums) pinned to
textbook_util.hmm_estep_torch on CPU tensors at one-hot and all-ones weights,
and to itself under an exact scaling of the weights."""
import ctypes as C

import numpy as np
import pytest

import nip_amd
from nip_amd import synth

import estep_soft_util as es
import soft_util as so

torch = pytest.importorskip("torch")
from textbook_util import hmm_estep_torch  # noqa: E402

NAMES = ["nipamd_estep_soft_partial", "nipamd_estep_soft", "nipamd_estep_soft_host"]
UNSUPPORTED, INVALID, NULL = nip_amd.NIPAMD_ERROR_UNSUPPORTED, nip_amd.NIP_ERROR_INVALID_ARGUMENT, \
    nip_amd.NIP_ERROR_NULLPOINTER


def spec_model(spec):
    nodes, pots = spec
    return nip_amd.Model.from_spec(nodes, pots)


def call(name, m, obs_vars, soft_vars, B=2, T=3, handle=True, obs=True, lik=True, ov_ptr=True, sv_ptr=True, out=True):
    """One of the entry points on host buffers of the right size (the device
    forms only test them for NULL before they refuse or fail: every case here
    ends before a kernel could read them)."""
    L = nip_amd.lib()
    card = lambda v: max(m.card(v), 1) if 0 <= v < m.num_vars else 1
    nb, nt = max(B, 1), max(T, 1)
    o = np.zeros((nb, nt, max(len(obs_vars), 1)), np.int32)
    w = np.ones((nb, nt, max(sum(card(v) for v in soft_vars), 1)))
    n_out = max(m.param_size(), L.nipamd_estep_partial_size(m._h), 1)
    c = np.ones(n_out)
    ll, st = np.zeros(nb), np.zeros(nb, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [m._h if handle else None, ptr(o) if obs else None, len(obs_vars), nip_amd._ints(obs_vars) if ov_ptr else None,
            ptr(w) if lik else None, len(soft_vars), nip_amd._ints(soft_vars) if sv_ptr else None, B, T,
            ptr(c) if out else None, ptr(ll), ptr(st)]
    if not name.endswith("_host"):
        args.append(None)
    return getattr(L, name)(*args)


def unsupported(rc):
    assert rc == UNSUPPORTED, rc
    msg = nip_amd.lib().nipamd_last_error().decode()
    assert msg.strip()
    return msg


def five_children():
    nodes = [("P0", 3, "P1"), ("P1", 3, None)] + [("O%d" % k, 2, None) for k in range(5)]
    pots = [("P1", ["P0"], synth.cpt(1, 3, 3)), ("P0", [], synth.cpt(2, 3, 1))]
    pots += [("O%d" % k, ["P1"], synth.cpt(3 + k, 2, 3)) for k in range(5)]
    w = nip_amd.Model.from_spec(nodes, pots)
    return w, [w.variable("O%d" % k) for k in range(5)]


def test_symbols_exported():
    L = C.CDLL(nip_amd.LIB_PATH)
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in nip_amd.EXPORTS
    for f in ("e_step_soft", "estep_partial_soft", "e_step_soft_host", "em_learn_soft"):
        assert callable(getattr(nip_amd, f)) and f in nip_amd.__all__


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors(name):
    m = spec_model(synth.hmm_spec(3, 4))
    M1 = m.variable("M1")
    for engine in (nip_amd.ENGINE_AUTO, nip_amd.ENGINE_JTREE):         # the arguments are decided before the scope
        m.set_engine(engine)
        assert call(name, m, [], [M1], handle=False) == NULL
        assert call(name, m, [M1], [], ov_ptr=False) == NULL
        assert call(name, m, [], [M1], sv_ptr=False) == NULL
        assert call(name, m, [], [M1], lik=False) == NULL
        assert call(name, m, [M1], [], obs=False) == NULL
        assert call(name, m, [], [M1], out=False) == NULL
        assert call(name, m, [], [M1], B=0) == INVALID
        assert call(name, m, [], [M1], T=0) == INVALID
        assert call(name, m, [], [M1], B=-3) == INVALID
        for bad in (99, -1):
            assert call(name, m, [bad], [M1]) == INVALID
            assert call(name, m, [], [bad]) == INVALID


@pytest.mark.parametrize("name", NAMES)
def test_scope_refusals(name):
    n = spec_model(synth.nonleaf_spec())
    assert "chain" in unsupported(call(name, n, [], [n.variable("Q1")]))
    m = spec_model(synth.hmm_spec(3, 4))
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    m.set_engine(nip_amd.ENGINE_JTREE)
    assert "JTREE" in unsupported(call(name, m, [], [M1]))
    m.set_engine(nip_amd.ENGINE_AUTO)
    assert "hard and as soft" in unsupported(call(name, m, [M1], [M1]))
    unsupported(call(name, m, [], [M1, M1]))                           # twice in soft_vars
    unsupported(call(name, m, [], [P0]))                               # neither the interface nor a leaf child
    assert "interface variable itself" in unsupported(call(name, m, [], [P1]))
    assert "interface variable itself" in unsupported(call(name, m, [P1], [M1]))
    w, ov = five_children()
    assert "four" in unsupported(call(name, w, ov[:3], ov[3:]))       # 3 hard + 2 soft
    assert "leaf children" in unsupported(call(name, w, [], ov[:1]))  # five children: no wide e_step plan
    f = spec_model(synth.factorial_spec(4, 4, 5))
    assert "joint interface" in unsupported(call(name, f, [], [f.variable("O1")]))


@pytest.mark.parametrize("name", NAMES)
def test_lds_need_beyond_a_cu(name):
    """16 states and an 80-state soft child: the count tables of a block -- 82
    rows of 128 bytes for each of its 16 sequences, 167936 bytes -- are more
    than a CU's 160 KB on their own."""
    m = spec_model(synth.hmm_spec(16, 80))
    msg = unsupported(call(name, m, [], [m.variable("M1")], B=1, T=1))
    assert "LDS" in msg and "bytes" in msg


@pytest.mark.parametrize("name", ["nipamd_estep_soft_host"])
def test_a_request_in_scope_passes_the_host_verdict(name):
    """Everything in scope: the call runs where there is a GPU, and fails with
    the device error -- not a refusal -- where there is none."""
    ok = (0, nip_amd.NIPAMD_ERROR_DEVICE)
    m = spec_model(synth.hmm_spec(3, 4))
    M1 = m.variable("M1")
    assert call(name, m, [], [M1]) in ok
    assert call(name, m, [M1], []) in ok                               # n_soft == 0: hard columns only
    assert call(name, m, [], []) in ok


def test_python_input_checks():
    """The wrappers refuse inputs the kernel could not read through their raw
    pointers, before any launch (CPU tensors here: nothing could run)."""
    m = spec_model(synth.hmm_spec(3, 4))
    M1 = m.variable("M1")
    lik = torch.ones((2, 3, 4), dtype=torch.float64)
    for fn in (nip_amd.e_step_soft, nip_amd.estep_partial_soft):
        with pytest.raises(nip_amd.NipError) as e:
            fn(m, None, [], lik, [M1])                                 # not on the device
        assert e.value.code == INVALID
        with pytest.raises(nip_amd.NipError):
            fn(m, None, [], None, [M1])
        with pytest.raises(nip_amd.NipError):
            fn(m, None, [], None, [])
    with pytest.raises(nip_amd.NipError) as e:
        nip_amd.e_step_soft_host(m, None, [], np.ones((2, 3, 5)), [M1])   # W = 4
    assert e.value.code == INVALID
    with pytest.raises(nip_amd.NipError) as e:
        nip_amd.e_step_soft_host(m, np.zeros((2, 4, 1), np.int32), [M1], np.ones((2, 3, 4)), [M1])
    assert e.value.code == INVALID
    with pytest.raises(nip_amd.NipError) as e:
        nip_amd.e_step_soft_host(m, None, [], np.ones((2, 3, 4)), [M1], counts=np.ones(3))
    assert e.value.code == INVALID


# ---------------------------------------------------------------------------
# the oracle, pinned to the textbook e_step

def tables(N, M, seed):
    rng = np.random.default_rng(seed)
    A = rng.random((N, N)) + 0.05
    A /= A.sum(axis=1, keepdims=True)
    pi = rng.random(N) + 0.05
    pi /= pi.sum()
    E = rng.random((N, M)) + 0.05                                  # rows do not sum to 1: the ll's m1 term matters
    return rng, A, pi, E


B_, T_, M_ = 4, 12, 5
PIN = 1e-12      # both sides fp64 on the CPU, sums of B_ T_ = 48 terms of at most 1


def hmm_layout(A, E, sums):
    K, Hs, P0 = sums[:3]
    p0, trans, kids = es.star_blocks(A, [E], K, Hs, P0)
    return np.concatenate([p0, trans, kids[0]])


def textbook(A, pi, E, codes):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    cnt, ll = hmm_estep_torch(t(A), t(pi), t(E), t(codes).long())
    return cnt.numpy(), ll.numpy()


@pytest.mark.parametrize("N", [3, 16])
def test_one_hot_weights_are_hard_observations(N):
    rng, A, pi, E = tables(N, M_, 160 + N)
    codes = rng.integers(0, M_, size=(B_, T_))
    want, want_ll = textbook(A, pi, E, codes)
    for kinds, cols, liks in (([so.SOFT], [None], [np.eye(M_)[codes]]), ([so.HARD], [codes], [None])):
        sums = es.soft_sums(A, pi, [E], kinds, cols, liks)
        assert np.abs(hmm_layout(A, E, sums) - want).max() <= PIN
        assert np.abs(sums[3] - want_ll).max() <= PIN * np.abs(want_ll).max()
        assert np.all(sums[4] == 0)
    # the soft child's own rows hold the counts; its missing and out-of-range rows stay empty
    H = es.soft_sums(A, pi, [E], [so.SOFT], [None], [np.eye(M_)[codes]])[1][0]
    assert np.all(H[:, M_:] == 0.0) and H[:, :M_].sum() == pytest.approx(B_ * T_, rel=1e-13)


@pytest.mark.parametrize("N", [3, 16])
def test_all_ones_weights_are_missing_observations(N):
    rng, A, pi, E = tables(N, M_, 170 + N)
    codes = rng.integers(0, M_, size=(B_, T_))
    codes[rng.random(codes.shape) < 0.4] = -1
    codes[0] = -1
    want, want_ll = textbook(A, pi, E, codes)
    sums = es.soft_sums(A, pi, [E], [so.SOFT], [None], [es.one_hot(codes, M_)])
    assert np.abs(hmm_layout(A, E, sums) - want).max() <= PIN
    assert np.abs(sums[3] - want_ll).max() <= PIN * max(1.0, np.abs(want_ll).max())
    hard = es.soft_sums(A, pi, [E], [so.HARD], [codes], [None])
    assert np.abs(hmm_layout(A, E, hard) - want).max() <= PIN
    # a hard column beside the soft one, and a child that no column names
    E2 = rng.random((N, 3)) + 0.05
    c2 = rng.integers(-1, 3, size=(B_, T_))
    none = np.full((B_, T_), -1)
    a = es.soft_sums(A, pi, [E, E2], [so.SOFT, so.HARD], [None, c2], [np.ones((B_, T_, M_)), None])
    b = es.soft_sums(A, pi, [E, E2], [so.HARD, so.HARD], [none, c2], [None, None])
    pa, pb = es.star_blocks(A, [E, E2], a[0], a[1], a[2]), es.star_blocks(A, [E, E2], b[0], b[1], b[2])
    for x, y in zip([pa[0], pa[1]] + pa[2], [pb[0], pb[1]] + pb[2]):
        assert np.abs(x - y).max() <= PIN


@pytest.mark.parametrize("N", [3, 16])
def test_scaling_by_powers_of_two_moves_only_the_ll(N):
    rng, A, pi, E = tables(N, M_, 190 + N)
    w = 0.05 + rng.random((B_, T_, M_))
    j = rng.integers(-900, 901, size=(B_, T_))
    base = es.soft_sums(A, pi, [E], [so.SOFT], [None], [w])
    got = es.soft_sums(A, pi, [E], [so.SOFT], [None], [np.ldexp(w, j[:, :, None])])
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1][0], base[1][0]) and np.array_equal(got[2], base[2])
    shift = j.sum(axis=1) * np.log(2.0)
    assert np.all(np.abs(got[3] - base[3] - shift) <= 1e-12 * np.maximum(1.0, np.abs(shift)))


def test_dead_sequences_and_bad_weights():
    rng, A, pi, E = tables(3, M_, 199)
    w = 0.05 + rng.random((B_, T_, M_))
    good = es.soft_sums(A, pi, [E], [so.SOFT], [None], [w])
    assert np.all(good[4] == 0)
    for value, status in ((0.0, 3), (np.nan, 7), (-1.0, 7), (np.inf, 7)):
        wb = w.copy()
        if value == 0.0:
            wb[1, 3] = 0.0
        else:
            wb[1, 3, 2] = value
        K, Hs, P0, ll, st = es.soft_sums(A, pi, [E], [so.SOFT], [None], [wb])
        assert list(st) == [0, status, 0, 0]
        assert ll[1] == -np.finfo(np.float64).max
        assert np.all(K[1] == 0.0) and np.all(Hs[0][1] == 0.0) and np.all(P0[1] == 0.0)
        for k in (0, 2, 3):
            assert np.array_equal(K[k], good[0][k]) and np.array_equal(Hs[0][k], good[1][0][k])
        assert not np.isnan(K).any() and not np.isnan(Hs[0]).any() and not np.isnan(P0).any()
