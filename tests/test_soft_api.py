"""Soft (likelihood) evidence (nipamd_fb_soft, nipamd_filter_soft and their
host forms) without a GPU: the exported symbols, the argument and scope
verdicts (decided on the host, before anything touches the device), and the
numpy oracle of tests/test_gpu_soft.py (soft_util.soft_smoother) pinned to
textbook_util.smoother and, on the inputs of tests/test_gpu_soft_scale.py
(weights from denormal to DBL_MAX), to a wide-exponent evaluation of the same
recursion that takes no scale out of anything (wide_smoother below)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nip_amd
from nip_amd import synth

import small_mass_util as sm
import soft_scale_util as ssu
import soft_util as so
from textbook_util import smoother

HOST = ["nipamd_fb_soft_host", "nipamd_filter_soft_host"]
NAMES = ["nipamd_fb_soft", "nipamd_filter_soft", "nipamd_fb_soft_host", "nipamd_filter_soft_host"]


def spec_model(spec):
    nodes, pots = spec
    return nip_amd.Model.from_spec(nodes, pots)


def call(name, m, obs_vars, soft_vars, query, B=2, T=3, handle=True, obs=True, lik=True, ov_ptr=True, sv_ptr=True,
         q_ptr=True, post=True):
    """One of the four entry points on host buffers of the right size (the
    device forms only test them for NULL before they refuse or fail: every
    case here ends before a kernel could read them, there being no GPU, or
    runs on a GPU's host form)."""
    L = nip_amd.lib()
    card = lambda v: max(m.card(v), 1) if 0 <= v < m.num_vars else 1
    o = np.zeros((B if B > 0 else 1, T if T > 0 else 1, max(len(obs_vars), 1)), np.int32)
    w = np.ones((B if B > 0 else 1, T if T > 0 else 1, max(sum(card(v) for v in soft_vars), 1)))
    p = np.zeros((B if B > 0 else 1, T if T > 0 else 1, max(sum(card(v) for v in query), 1)))
    ll, st = np.zeros(max(B, 1)), np.zeros(max(B, 1), np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [m._h if handle else None, ptr(o) if obs else None, len(obs_vars), nip_amd._ints(obs_vars) if ov_ptr else None,
            ptr(w) if lik else None, len(soft_vars), nip_amd._ints(soft_vars) if sv_ptr else None, B, T, len(query),
            nip_amd._ints(query) if q_ptr else None, ptr(p) if post else None, ptr(ll), ptr(st)]
    if not name.endswith("_host"):
        args.append(None)
    return getattr(L, name)(*args)


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
    for s in NAMES:
        assert hasattr(L, s), s
        assert s in nip_amd.EXPORTS
    for f in ("forward_backward_inference_soft", "forward_inference_soft", "forward_backward_inference_soft_host",
              "forward_inference_soft_host"):
        assert callable(getattr(nip_amd, f)) and f in nip_amd.__all__
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nip_amd.h")).read()
    assert int(re.search(r"#define\s+NIPAMD_STATUS_BAD_EVIDENCE\s+(\d+)u", hdr).group(1)) == nip_amd.STATUS_BAD_EVIDENCE
    assert nip_amd.STATUS_BAD_EVIDENCE == 4


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
        assert call(name, m, [], [M1], [P1], post=False) == NULL
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
    unsupported(call(name, m, [M1], [M1], [P1]))                       # in both lists
    unsupported(call(name, m, [], [M1, M1], [P1]))                     # twice in soft_vars
    unsupported(call(name, m, [M1, M1], [], [P1]))                     # twice in obs_vars
    unsupported(call(name, m, [], [P0], [P1]))                         # neither the interface nor a leaf child
    w, ov, wP1 = five_children()
    assert "four" in unsupported(call(name, w, ov[:3], ov[3:], [wP1]))  # 3 hard + 2 soft
    for q in ([M1], [P0], [P1, P1], []):
        assert "interface" in unsupported(call(name, m, [], [M1], q)), q


@pytest.mark.parametrize("name", NAMES)
def test_lds_need_beyond_a_cu(name):
    """64 states and four soft children of 64 states each: 4 x 66 table rows of
    512 bytes and two 32 KB images of A are more than a CU's 160 KB."""
    nodes = [("P0", 64, "P1"), ("P1", 64, None)] + [("O%d" % k, 64, None) for k in range(4)]
    pots = [("P1", ["P0"], synth.cpt(1, 64, 64)), ("P0", [], synth.cpt(2, 64, 1))]
    pots += [("O%d" % k, ["P1"], synth.cpt(3 + k, 64, 64)) for k in range(4)]
    w = nip_amd.Model.from_spec(nodes, pots)
    ov = [w.variable("O%d" % k) for k in range(4)]
    assert "LDS" in unsupported(call(name, w, [], ov, [w.variable("P1")], B=1, T=1))
    if name in HOST:                                                   # (host buffers: no device form in scope)
        assert call(name, w, [], ov[:1], [w.variable("P1")], B=1, T=1) in (0, nip_amd.NIPAMD_ERROR_DEVICE)


@pytest.mark.parametrize("name", HOST)
def test_a_request_in_scope_passes_the_host_verdict(name):
    """Everything in scope: the call runs where there is a GPU, and fails with
    the device error -- not a refusal -- where there is none.  (The host forms:
    their buffers are real whichever it is.)"""
    ok = (0, nip_amd.NIPAMD_ERROR_DEVICE)
    m = spec_model(synth.hmm_spec(3, 4))
    P1, M1 = m.variable("P1"), m.variable("M1")
    assert call(name, m, [], [M1], [P1]) in ok
    assert call(name, m, [], [P1], [P1]) in ok                         # the interface variable itself
    assert call(name, m, [M1], [P1], [P1]) in ok
    assert call(name, m, [], [], [P1]) in ok
    w, ov, wP1 = five_children()
    assert call(name, w, ov[:2], ov[2:4], [wP1]) in ok
    f = spec_model(synth.factorial_spec(4, 4, 5))
    X1, Y1, O1 = f.variable("X1"), f.variable("Y1"), f.variable("O1")
    for q in ([X1, Y1], [Y1]):
        assert call(name, f, [], [O1], q) in ok


# ---------------------------------------------------------------------------
# the oracle, pinned to the textbook smoother

def tables(N, M, seed, proper=False):
    rng = np.random.default_rng(seed)
    A = rng.random((N, N)) + 0.05
    A /= A.sum(axis=1, keepdims=True)
    pi = rng.random(N) + 0.05
    pi /= pi.sum()
    E = rng.random((N, M)) + 0.05                                  # rows do not sum to 1: the ll's m1 term matters
    if proper:
        E /= E.sum(axis=1, keepdims=True)
    return rng, A, pi, E


B_, T_, M_ = 4, 12, 5


def soft1(A, pi, E, w):
    return so.soft_smoother(A, pi, [E], [so.SOFT], [None], [w])


@pytest.mark.parametrize("N", [3, 16])
def test_one_hot_weights_are_hard_observations(N):
    rng, A, pi, E = tables(N, M_, 60 + N)
    codes = rng.integers(0, M_, size=(B_, T_))
    want = smoother(A, pi, [E], [codes])
    got = soft1(A, pi, E, np.eye(M_)[codes])
    for g, w in zip(got, want):
        assert np.abs(g - w).max() <= 1e-13


@pytest.mark.parametrize("N", [3, 16])
def test_all_ones_weights_are_missing_observations(N):
    rng, A, pi, E = tables(N, M_, 70 + N)
    want = smoother(A, pi, [E], [np.full((B_, T_), -1)])
    got = soft1(A, pi, E, np.ones((B_, T_, M_)))
    for g, w in zip(got, want):
        assert np.abs(g - w).max() <= 1e-13
    # and a hard column beside a soft one, each on its own table
    E2 = rng.random((N, 3)) + 0.05
    codes = rng.integers(-1, 3, size=(B_, T_))
    want = smoother(A, pi, [E, E2], [np.full((B_, T_), -1), codes])
    got = so.soft_smoother(A, pi, [E, E2], [so.SOFT, so.HARD], [None, codes], [np.ones((B_, T_, M_)), None])
    for g, w in zip(got, want):
        assert np.abs(g - w).max() <= 1e-13


@pytest.mark.parametrize("N", [3, 16])
def test_mixture_identity(N):
    """Random weights at one step t*, hard codes elsewhere: the evidence is the
    w-mixture of the M hard sequences, so exp(ll) = sum_o w_o exp(ll_o) and the
    rows are the mixture of the rows under weights w_o exp(ll_o).  Both sides
    fp64 numpy at T = 12: rows 1e-12, ll 1e-12 max(1, |ll|).  The tables are
    proper here (every m1 is 1 and ll = log P(evidence), which is what mixes
    linearly: under improper emission rows m1_t depends on alpha^_{t-1} and the
    ll is no mixture, while the rows still are)."""
    rng, A, pi, E = tables(N, M_, 80 + N, proper=True)
    codes = rng.integers(0, M_, size=(B_, T_))
    ts = 7
    w = np.eye(M_)[codes]
    wt = 0.05 + rng.random((B_, M_))
    w[:, ts] = wt
    post, filt, ll = soft1(A, pi, E, w)
    num_p, num_f, den = 0.0, 0.0, 0.0
    for o in range(M_):
        c = codes.copy()
        c[:, ts] = o
        post_o, filt_o, ll_o = smoother(A, pi, [E], [c])
        k = wt[:, o] * np.exp(ll_o)
        num_p = num_p + k[:, None, None] * post_o
        den = den + k
        num_f = num_f + k[:, None, None] * filt_o
    want_ll = np.log(den)
    assert np.all(np.abs(ll - want_ll) <= 1e-12 * np.maximum(1.0, np.abs(want_ll)))
    assert np.abs(post - num_p / den[:, None, None]).max() <= 1e-12
    # the filtered rows before t* do not see the soft step; the last one is the smoothed one
    assert np.abs(filt[:, -1] - (num_f / den[:, None, None])[:, -1]).max() <= 1e-12
    assert np.abs(filt[:, :ts] - smoother(A, pi, [E], [codes])[1][:, :ts]).max() <= 1e-13


@pytest.mark.parametrize("N", [3, 16])
def test_scaling_a_step_moves_only_the_ll(N):
    rng, A, pi, E = tables(N, M_, 90 + N)
    w = 0.05 + rng.random((B_, T_, M_))
    post, filt, ll = soft1(A, pi, E, w)
    w2 = w.copy()
    w2[:, 4] *= 7.5
    post2, filt2, ll2 = soft1(A, pi, E, w2)
    assert np.abs(post2 - post).max() <= 1e-14 and np.abs(filt2 - filt).max() <= 1e-14
    assert np.all(np.abs(ll2 - ll - np.log(7.5)) <= 1e-12 * np.maximum(1.0, np.abs(ll)))


def test_dead_sequences_and_bad_weights():
    rng, A, pi, E = tables(3, M_, 99)
    w = 0.05 + rng.random((B_, T_, M_))
    good = soft1(A, pi, E, w)
    assert np.all(so.soft_status(A, pi, [E], [so.SOFT], [None], [w]) == 0)
    for value, status in ((0.0, 1), (np.nan, 5), (-1.0, 5), (np.inf, 5)):
        wb = w.copy()
        if value == 0.0:
            wb[1, 6] = 0.0
        else:
            wb[1, 6, 2] = value
        post, filt, ll = soft1(A, pi, E, wb)
        st = so.soft_status(A, pi, [E], [so.SOFT], [None], [wb])
        assert list(st) == [0, status, 0, 0]
        assert ll[1] == -np.finfo(np.float64).max and np.all(post[1] == 0.0)
        assert np.array_equal(filt[1, :6], good[1][1, :6]) and np.all(filt[1, 6:] == 0.0)
        assert not np.isnan(post).any() and not np.isnan(filt).any() and not np.isnan(ll).any()
        for k in (0, 2, 3):
            assert np.array_equal(post[k], good[0][k]) and ll[k] == good[2][k]


# ---------------------------------------------------------------------------
# the oracle at every weight scale, pinned to a wide-exponent evaluation
#
# wide_smoother is the recursion of soft_util._run written out again with the
# weights as given -- no exponent taken out, e_t the plain product -- in a
# number format whose exponent range holds every product these inputs form
# (four columns at DBL_MAX: 2^4096): np.longdouble where it is the x87 80-bit
# format (maxexp 16384, 64-bit mantissa), mpmath at 50 digits elsewhere.

def wide_backend():
    return "longdouble" if np.finfo(np.longdouble).maxexp > 1024 else "mpmath"


def wide_ops(backend):
    """(to, log, back): float64 array -> wide array, the elementwise logarithm
    of positive wide numbers, wide array -> float64."""
    if backend == "longdouble":
        return (lambda a: np.asarray(a, np.longdouble)), np.log, (lambda a: np.asarray(a, np.float64))
    import mpmath
    ctx = mpmath.MPContext()
    ctx.dps = 50
    to = np.frompyfunc(lambda x: ctx.mpf(float(x)), 1, 1)
    log = np.frompyfunc(ctx.log, 1, 1)
    back = lambda a: np.frompyfunc(float, 1, 1)(a).astype(np.float64)
    return (lambda a: to(np.asarray(a, np.float64))), log, back


def wide_smoother(A, pi, Es, kinds, cols, liks, backend=None):
    """(smoothed, filtered, ll, status) as float64 / int64 arrays, soft_util's
    definitions (a dead sequence: ll = -DBL_MAX, zero rows from its dead step
    on, all smoothed rows zero; status 1, plus 4 for a bad weight)."""
    to, log, back = wide_ops(backend or wide_backend())
    Aw, Ew = to(A), [to(E) for E in Es]
    T = next(c.shape[1] for kind, c in zip(kinds, cols) if kind == so.HARD) if so.HARD in kinds else \
        next(w.shape[1] for kind, w in zip(kinds, liks) if kind == so.SOFT)
    B = next(c.shape[0] for kind, c in zip(kinds, cols) if kind == so.HARD) if so.HARD in kinds else \
        next(w.shape[0] for kind, w in zip(kinds, liks) if kind == so.SOFT)
    N = A.shape[0]
    zero, one = to(np.zeros((1, 1))), to(np.ones((1, 1)))
    s_all = one[0] * to(np.ones(N))
    for E in Ew:
        s_all = s_all * E.sum(axis=1)

    def ev(t):
        e = one * to(np.ones((B, N)))
        bad = np.zeros(B, bool)
        for E, kind, c, w in zip(Ew, kinds, cols, liks):
            if kind == so.HARD:
                x, M = c[:, t], E.shape[1]
                f = E[:, np.clip(x, 0, M - 1)].T
                f = np.where((x < 0)[:, None], E.sum(axis=1)[None, :], f)
                f = np.where((x >= M)[:, None], zero, f)
            else:
                wt = np.asarray(w[:, t], np.float64)
                wb = ~(np.isfinite(wt) & (wt >= 0.0))
                bad |= wb.any(axis=1)
                f = to(np.where(wb, 0.0, wt)) @ E.T
            e = e * f
        return np.where(bad[:, None], zero, e), bad

    evs = [ev(t) for t in range(T)]
    ah = []
    ll = to(np.zeros(B))
    status = np.zeros(B, np.int64)
    alive = np.ones(B, bool)
    prev = one * to(np.tile(pi, (B, 1)))
    for t in range(T):
        e, bad = evs[t]
        status[bad] |= 4
        u = prev @ Aw
        al = u * e
        c = al.sum(axis=1)
        alive &= np.asarray(c > 0, bool)
        c = np.where(alive, c, one[0])                          # a dead sequence divides by 1 and is zeroed
        m1 = np.where(alive, (u * s_all).sum(axis=1), one[0])
        ll = ll + np.where(alive, log(c) - log(m1), zero[0])
        prev = np.where(alive[:, None], al / c[:, None], zero)
        ah.append(prev)
    status[~alive] |= 1
    post = [None] * T
    post[T - 1] = ah[T - 1]
    b = one * to(np.ones((B, N)))
    for t in range(T - 2, -1, -1):
        b = (evs[t + 1][0] * b) @ Aw.T
        b = np.where(alive[:, None], b / np.where(alive, b.sum(axis=1), one[0])[:, None], zero)
        p = ah[t] * b
        post[t] = np.where(alive[:, None], p / np.where(alive, p.sum(axis=1), one[0])[:, None], zero)
    stack = lambda rows: np.stack([back(r) for r in rows], axis=1)
    post, filt, ll = stack(post), stack(ah), back(ll)
    post[~alive] = 0.0
    ll[~alive] = -np.finfo(np.float64).max
    return post, filt, ll, status


PIN_ROWS, PIN_LL, REF_MOVE = 1e-14, 1e-13, 1e-15


def usable(ref):
    """The conditions on an input: the reference alone gives every sequence
    mass and finite rows."""
    post, filt, ll, status = ref
    assert np.all(status == 0), status.tolist()
    assert np.isfinite(post).all() and np.isfinite(filt).all() and np.isfinite(ll).all()


def pinned(got, ref, what):
    """The fp64 oracle against the reference."""
    for g in got[:3]:
        assert np.isfinite(g).all(), what
    rows = max(np.abs(got[0] - ref[0]).max(), np.abs(got[1] - ref[1]).max())
    lerr = (np.abs(got[2] - ref[2]) / np.maximum(1.0, np.abs(ref[2]))).max()
    print("%s: oracle against the wide reference: rows %.3g, ll %.3g (relative)" % (what, rows, lerr))
    assert rows <= PIN_ROWS, (what, rows)
    assert lerr <= PIN_LL, (what, lerr)
    assert np.array_equal(got[3], ref[3]), what


@pytest.mark.parametrize("T", ssu.TS)
@pytest.mark.parametrize("name", ssu.NAMES)
def test_oracle_at_every_weight_scale(name, T):
    """Every input of tests/test_gpu_soft_scale.py's scale grid: usable by the
    reference alone, the reference's rows unmoved by the scaling (1e-15), and
    the fp64 oracle on the reference (rows 1e-14, ll 1e-13 max(1, |ll|), the
    same status, everything finite)."""
    r = ssu.requests()[name]
    A, pi, Es = r.tables
    obs, base = ssu.hard_obs(r, T), ssu.base_weights(r, T)

    def both(liks):
        args = ssu.oracle_args(r, obs, liks)
        ref = wide_smoother(A, pi, Es, *args)
        usable(ref)
        return so._run(A, pi, Es, *args), ref

    got0, ref0 = both(base)
    pinned(got0, ref0, "unscaled")
    for big in (560, 530) if name in ssu.TWO_COLUMN else (560,):
        k = ssu.exponents(T, len(r.soft), big)
        got, ref = both(ssu.scaled(base, k))
        move = max(np.abs(ref[0] - ref0[0]).max(), np.abs(ref[1] - ref0[1]).max())
        print("big = %d: the scaling moves the reference's rows by %.3g" % (big, move))
        assert move <= REF_MOVE, move
        pinned(got, ref, "big = %d" % big)
        # and the oracle's own rows do not see an exact scaling at all
        assert np.array_equal(got[0], got0[0]) and np.array_equal(got[1], got0[1])
    pinned(*both(ssu.edge_weights(r, T)), "the edge batch")


def test_wide_reference_formats_agree():
    """The mpmath form of the reference, which a machine whose long double is
    no wider than double runs, against the long double form where that exists
    (and against the fp64 oracle on an input of ordinary size elsewhere)."""
    r = ssu.requests()["demo20-both"]
    A, pi, Es = r.tables
    T = 5
    liks = ssu.scaled(ssu.base_weights(r, T), ssu.exponents(T, 2))
    args = ssu.oracle_args(r, ssu.hard_obs(r, T), liks)
    mp = wide_smoother(A, pi, Es, *args, backend="mpmath")
    usable(mp)
    other = wide_smoother(A, pi, Es, *args, backend="longdouble") if wide_backend() == "longdouble" else \
        so._run(A, pi, Es, *args)
    pinned(other, mp, "mpmath against " + wide_backend())


def fed_rows(T=64):
    """Smoothed rows of test_gpu_soft.two_blocks() under hard evidence: exact
    zeros on the second block and, towards the end, a shrinking first-block
    state -- the kind of rows test_gpu_soft_scale feeds back from the device."""
    import test_gpu_soft as tg
    _, _, _, (A, pi, Es) = tg.two_blocks()
    codes = tg.gappy(3, T, (4,), 91)[:, :, 0]
    codes[codes > 1] -= 2                                   # the first block's symbols
    return smoother(A, pi, Es, [codes])[0]


@pytest.mark.parametrize("shift", [0, -700])
def test_oracle_on_fed_back_rows(shift):
    import test_gpu_soft as tg
    _, _, _, (A, pi, Es) = tg.hmm(4, 4, True)
    fed = np.ldexp(fed_rows(), shift)
    assert np.all(fed[:, :, 2:] == 0.0) and np.all(fed[:, :, :2].max(axis=2) > 0.0)
    args = ([so.HARD, so.SOFT], [np.full(fed.shape[:2], -1), None], [None, fed])
    ref = wide_smoother(A, pi, Es + [np.eye(4)], *args)
    usable(ref)
    pinned(so._run(A, pi, Es + [np.eye(4)], *args), ref, "fed rows 2^%d" % shift)


@pytest.mark.parametrize("mu", [1e-80, 1e-150])
def test_oracle_on_rare_steps_as_weights(mu):
    """small_mass_util's rare steps as one-hot weights (all ones at a missing
    step) and with the first column soft beside hard ones: the oracle on the
    reference and on textbook_util.smoother (1e-13, as the pins above)."""
    T = 24
    for c in (sm.rare_hmm(16, 4, mu), sm.rare_star(17, sm.STAR_CARDS, sm.col_scale(mu, 4))):
        A, pi, Es = c.tables
        obs = sm.rare_obs(T, c.cards, B=ssu.B)
        cols = c.cols(obs)
        want = smoother(A, pi, Es, cols)
        hot = [np.where((x < 0)[:, :, None], 1.0, np.eye(E.shape[1])[np.maximum(x, 0)]) for E, x in zip(Es, cols)]
        n = len(Es)
        for nsoft in (n, 1):
            kinds = [so.SOFT] * nsoft + [so.HARD] * (n - nsoft)
            args = (kinds, [None] * nsoft + cols[nsoft:], hot[:nsoft] + [None] * (n - nsoft))
            ref = wide_smoother(A, pi, Es, *args)
            usable(ref)
            got = so._run(A, pi, Es, *args)
            pinned(got, ref, "mu = %g, %d soft of %d" % (mu, nsoft, n))
            for g, w in zip(got[:2], want[:2]):
                assert np.abs(g - w).max() <= 1e-13
            assert np.all(np.abs(got[2] - want[2]) <= 1e-13 * np.maximum(1.0, np.abs(want[2])))
