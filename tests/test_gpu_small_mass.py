"""Every chain route at tiny step masses.

The reference normalises its messages at every step and adds log m2 - log m1
to the ll per step, so its results do not depend on how small one step's
evidence mass is.  Several chain kernels rescale every 4th step only, and
almost all multiply four steps' masses into one mantissa before they take a
logarithm.  Both are sound while a step's mass stays moderate; the host's
bound (engine_route.cpp step_shrink_ok) decides, and this file runs each
route on both sides of it.

Inputs: tests/small_mass_util.py -- rare-symbol models whose code 0 has
probability s from every state in every observed child, so a step with all
ncol observed columns at code 0 has mass mu = s^ncol; mu = 1e-20, 1e-40,
1e-80, 1e-150, T = 24 and 37 (and 131 once, at 1e-80), B = 17 sequences with
rare runs at the start, the end, across T/2, everywhere, alternating with
missing steps, in runs of 3 and 4 across the rescale positions, and at random.
mu stops at 1e-150 because the oracles do (tests/test_small_mass_oracle.py
pins them to each other on these inputs).  Beside the proper models (every
row sums to 1) there are HMMs whose transition rows do not (the kernels'
general mode, where the ll is the sum of per-step terms), and the 16-state
e_step runs once more at 1e-66.

Before the bound routed these requests, every case passed at 1e-20 and 1e-40
and these failed at 1e-80 and 1e-150, at every T: smoothing on
chain_fb_ckpt_kernel (plain and <proj>), chain_fb_mfma_kernel and
chain_row64_kernel (posteriors NaN, 0.06-0.46 off at 1e-150; ll 2e-7..8e-6
relative off, -DBL_MAX at 1e-150), filtering on chain_row64_kernel (the same)
and chain_mfma_wide_kernel (ll only: 2e-7..4e-7, NaN at 1e-150), the e_step on
chain_estep16_kernel (counts NaN, also at 1e-66).  chain_mfma_wide_kernel's
smoothing, chain_estep_mw_kernel, the two-kernel wide e_step, op_fb_kernel, the
general engine, chain_viterbi_kernel and chain_stream_kernel passed throughout.

Expectations, the project's own: status 0 everywhere (every sequence has
mass), posteriors and rows 1e-12 absolute, ll 1e-11 max(1, |ll|), counts 1e-11
relative (em_util.close), mlss as test_gpu_viterbi.check, streams as
test_gpu_stream.check_rows / check_ll.  The last test pins (operation, model,
mu) -> nip_amd.last_kernel().
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import nip_amd
from oracle.bind import PortOracle

import small_mass_util as sm
import stream_util as su
from em_util import close
from textbook_util import smoother

import test_gpu_stream as tgs
import test_gpu_viterbi as tgv

DBL_MAX = np.finfo(np.float64).max
B = sm.B
PTOL, LTOL, CTOL = 1e-12, 1e-11, 1e-11
GRID = [(mu, T) for mu in sm.MUS for T in (24, 37)] + [(1e-80, 131)]
GRID_IDS = ["%g-T%d" % g for g in GRID]

CKPT, PROJ, MFMA = "chain_fb_ckpt_kernel", "chain_fb_ckpt_kernel<proj>", "chain_fb_mfma_kernel"
FBCK, MW1, MW2 = "chain_fb_ckw_kernel", "chain_mfma_wide_kernel<1>", "chain_mfma_wide_kernel<2>"
ROW64, WIDE64 = "chain_row64_kernel", "chain_wide_kernel<64>"
OP, JT = "op_fb_kernel", "jt_filter_kernel + jt_post_kernel"
VIT, STREAM = "chain_viterbi_kernel", "chain_stream_kernel"
ECK, E16, ECKW, EMW = "chain_estep_ck_kernel", "chain_estep16_kernel", "chain_estep_ckw_kernel", "chain_estep_mw_kernel"
EMSGS = "chain_msgs_kernel + chain_stats_kernel"

# name -> (builder of the Case at step mass mu, engine)
MODELS = {
    "hmm13": (lambda mu: sm.rare_hmm(13, 4, mu), nip_amd.ENGINE_AUTO),
    "hmm16": (lambda mu: sm.rare_hmm(16, 4, mu), nip_amd.ENGINE_AUTO),
    "hmm20": (lambda mu: sm.rare_hmm(20, 4, mu), nip_amd.ENGINE_AUTO),
    "hmm40": (lambda mu: sm.rare_hmm(40, 4, mu), nip_amd.ENGINE_AUTO),
    "hmm64": (lambda mu: sm.rare_hmm(64, 4, mu), nip_amd.ENGINE_AUTO),
    "demo16": (lambda mu: sm.rare_demo(16, sm.col_scale(mu, 2)), nip_amd.ENGINE_AUTO),
    "demo20": (lambda mu: sm.rare_demo(20, sm.col_scale(mu, 2)), nip_amd.ENGINE_AUTO),
    "demo40": (lambda mu: sm.rare_demo(40, sm.col_scale(mu, 2)), nip_amd.ENGINE_AUTO),
    "star17x3": (lambda mu: sm.rare_star(17, sm.STAR_CARDS, sm.col_scale(mu, 3), (2, 0, 3)), nip_amd.ENGINE_AUTO),
    "star17x4": (lambda mu: sm.rare_star(17, sm.STAR_CARDS, sm.col_scale(mu, 4)), nip_amd.ENGINE_AUTO),
    "star40x3": (lambda mu: sm.rare_star(40, sm.STAR_CARDS, sm.col_scale(mu, 3), (2, 0, 3)), nip_amd.ENGINE_AUTO),
    "star40x4": (lambda mu: sm.rare_star(40, sm.STAR_CARDS, sm.col_scale(mu, 4)), nip_amd.ENGINE_AUTO),
    "factorial445": (lambda mu: sm.rare_factorial(4, 4, 5, mu), nip_amd.ENGINE_AUTO),
    "nonleaf5": (lambda mu: sm.rare_nonleaf(5, 3, 3, mu), nip_amd.ENGINE_AUTO),
    # the control: the general engine normalises every step (its own model instance: the engine is a model setting)
    "hmm16_jtree": (lambda mu: sm.rare_hmm(16, 4, mu, seed=1), nip_amd.ENGINE_JTREE),
    # transition rows that do not sum to 1: the kernels' general mode, where the ll is the sum of the
    # per-step log m2 - log m1 and not the logarithm of the final mass
    "hmm16np": (lambda mu: sm.rare_hmm(16, 4, mu, proper=False), nip_amd.ENGINE_AUTO),
    "hmm20np": (lambda mu: sm.rare_hmm(20, 4, mu, proper=False), nip_amd.ENGINE_AUTO),
    "hmm40np": (lambda mu: sm.rare_hmm(40, 4, mu, proper=False), nip_amd.ENGINE_AUTO),
    "hmm64np": (lambda mu: sm.rare_hmm(64, 4, mu, proper=False), nip_amd.ENGINE_AUTO),
}
SMOOTH = ["hmm16", "hmm13", "hmm20", "hmm40", "demo16", "demo20", "demo40", "star17x3", "star17x4", "star40x3",
          "star40x4", "factorial445", "nonleaf5", "hmm16_jtree", "hmm16np", "hmm20np", "hmm40np"]
FILTER = ["hmm16", "hmm20", "hmm40", "star40x4", "hmm16np", "hmm40np"]
ESTEP = ["hmm16", "demo16", "demo20", "hmm64", "factorial445", "hmm16np", "hmm20np", "hmm64np"]
MLSS = ["hmm16", "hmm20", "hmm40", "star17x4"]
STREAMS = ["hmm16", "hmm20", "hmm40"]
NEAR, MU_NEAR = ["hmm16", "demo16", "factorial445", "hmm16np"], 1e-66

# (operation, model) -> the kernel at every mu, or one per mu of sm.MUS
def below(first, rest):
    """`first` at mu = 1e-20, above the step-shrink bound (1e-30), `rest` below it."""
    return (first, rest, rest, rest)


EXPECTED = {
    ("fb", "hmm16"): below(CKPT, MW1), ("fb", "hmm16np"): below(CKPT, MW1), ("fb", "hmm13"): below(MFMA, MW1),
    ("fb", "hmm20"): below(FBCK, MW2), ("fb", "hmm20np"): below(FBCK, MW2), ("fb", "demo20"): below(FBCK, MW2),
    ("fb", "hmm40"): below(ROW64, WIDE64), ("fb", "hmm40np"): below(ROW64, WIDE64),
    ("fb", "demo40"): below(ROW64, WIDE64), ("fb", "star40x3"): below(ROW64, WIDE64),
    ("fb", "star40x4"): below(ROW64, WIDE64),
    ("fb", "demo16"): MW1, ("fb", "star17x3"): MW2, ("fb", "star17x4"): MW2,
    ("fb", "factorial445"): below(PROJ, MW1), ("fb", "nonleaf5"): OP, ("fb", "hmm16_jtree"): JT,
    ("filter", "hmm16"): MW1, ("filter", "hmm16np"): MW1, ("filter", "hmm20"): MW2,
    ("filter", "hmm40"): below(ROW64, WIDE64), ("filter", "hmm40np"): below(ROW64, WIDE64),
    ("filter", "star40x4"): below(ROW64, WIDE64),
    # chain_estep16_kernel below the bound: its every-step mode, under the same name
    ("estep", "hmm16"): below(ECK, E16), ("estep", "hmm16np"): below(ECK, E16), ("estep", "demo16"): E16,
    ("estep", "factorial445"): E16, ("estep", "demo20"): below(ECKW, EMW), ("estep", "hmm20np"): below(ECKW, EMW),
    ("estep", "hmm64"): EMSGS, ("estep", "hmm64np"): EMSGS,
    ("mlss", "hmm16"): VIT, ("mlss", "hmm20"): VIT, ("mlss", "hmm40"): VIT, ("mlss", "star17x4"): VIT,
    ("stream", "hmm16"): STREAM, ("stream", "hmm20"): STREAM, ("stream", "hmm40"): STREAM,
}
EXPECTED_NEAR = {name: E16 for name in NEAR}    # e_step at MU_NEAR: model -> kernel

ROUTES = {}                            # (operation, model, mu) -> the kernels seen
_refs = {}


def case_of(name, mu):
    build, engine = MODELS[name]
    c = build(mu)
    c.m.set_engine(engine)
    return c


def reference(name, mu, T):
    """(obs, smoothed, filtered, ll) of the oracle, once per (model, mu, T):
    the textbook smoother over the model's own tables; the port oracle where
    the request is not a plain interface chain's (joint interface, non-leaf
    evidence)."""
    key = (name, mu, T)
    if key not in _refs:
        c = case_of(name, mu)
        obs = sm.rare_obs(T, c.cards)
        if name in ("factorial445", "nonleaf5"):
            orc = PortOracle(c.m.desc())
            post, ll = orc.fb_batch(obs, c.ov, c.q, nthreads=8)
            filt = None
        else:
            post, filt, ll = smoother(*c.tables, c.cols(obs))
        assert np.isfinite(post).all() and np.isfinite(ll).all() and (ll > -DBL_MAX).all()
        _refs[key] = (obs, post, filt, ll)
    return _refs[key]


def seen(op, name, mu):
    k = nip_amd.last_kernel()
    ROUTES.setdefault((op, name, mu), set()).add(k)
    return k


def check_post(where, gp, gl, gs, rp, rl):
    """A NaN counts as an infinite error."""
    perr = np.abs(gp - rp).reshape(B, -1).max(axis=1)
    lerr = np.abs(gl - rl) / np.maximum(1.0, np.abs(rl))
    perr, lerr = np.where(np.isnan(perr), np.inf, perr), np.where(np.isnan(lerr), np.inf, lerr)
    print("%s: posterior error %.3g, ll error %.3g (relative)" % (where, perr.max(), lerr.max()))
    bad = (perr > PTOL) | (lerr > LTOL) | (gs != 0)
    assert not bad.any(), "%s: sequences %s: posterior error %.3g, ll error %.3g (relative), ll %s, status %s" % (
        where, np.nonzero(bad)[0].tolist(), perr.max(), lerr.max(), gl[bad][:3].tolist(), gs[bad][:3].tolist())


def run_fb(name, mu, T, filt, check=True):
    """check=False (here and below): the request only, for its route."""
    c = case_of(name, mu)
    obs, post, fpost, ll = reference(name, mu, T)
    fn = nip_amd.forward_inference if filt else nip_amd.forward_backward_inference
    gp, gl, gs = fn(c.m, torch.from_numpy(obs).cuda(), c.ov, c.q)
    torch.cuda.synchronize()
    op = "filter" if filt else "fb"
    k = seen(op, name, mu)
    if not check:
        return
    check_post("%s %s mu=%g T=%d on %s" % (op, name, mu, T, k), gp.cpu().numpy(), gl.cpu().numpy(),
               gs.cpu().numpy(), fpost if filt else post, ll)


@pytest.mark.parametrize("mu,T", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("name", SMOOTH)
def test_smoothing(name, mu, T):
    run_fb(name, mu, T, False)


@pytest.mark.parametrize("mu,T", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("name", FILTER)
def test_filtering(name, mu, T):
    run_fb(name, mu, T, True)


def run_estep(name, mu, T, check=True):
    c = case_of(name, mu)
    key = ("estep", name, mu, T)
    obs = sm.rare_obs(T, c.cards)
    if not check:
        nip_amd.e_step(c.m, torch.from_numpy(obs).cuda(), c.ov)
        torch.cuda.synchronize()
        seen("estep", name, mu)
        return
    if key not in _refs:
        _refs[key] = PortOracle(c.m.desc()).estep(obs, c.ov, np.ones(c.m.param_size()))
    rc, rl, rb = _refs[key]
    assert not rb.any() and np.isfinite(rc).all()
    cnt, ll, st = nip_amd.e_step(c.m, torch.from_numpy(obs).cuda(), c.ov)
    torch.cuda.synchronize()
    k = seen("estep", name, mu)
    cnt, ll, st = cnt.cpu().numpy(), ll.cpu().numpy(), st.cpu().numpy()
    where = "estep %s mu=%g T=%d on %s" % (name, mu, T, k)
    cerr = np.abs(cnt - rc) / np.maximum(1.0, np.abs(rc))
    lerr = np.abs(ll - rl) / np.maximum(1.0, np.abs(rl))
    cerr, lerr = np.where(np.isnan(cerr), np.inf, cerr), np.where(np.isnan(lerr), np.inf, lerr)
    print("%s: count error %.3g, ll error %.3g (both relative)" % (where, cerr.max(), lerr.max()))
    assert not st.any(), "%s: status %s" % (where, st.tolist())
    assert close(ll, rl, LTOL), "%s: ll error %.3g (relative), sequences %s" % (
        where, lerr.max(), np.nonzero(lerr > LTOL)[0].tolist())
    assert close(cnt, rc, CTOL), "%s: count error %.3g (relative)" % (where, cerr.max())


@pytest.mark.parametrize("mu,T", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("name", ESTEP)
def test_estep(name, mu, T):
    run_estep(name, mu, T)


@pytest.mark.parametrize("T", [24, 37])
@pytest.mark.parametrize("name", NEAR)
def test_estep_between_the_matrix_points(name, T):
    """mu = 1e-66, between 1e-40 and 1e-80: chain_estep16_kernel with its
    backward rows rescaling every 4th step whatever the tables passed at 1e-40
    and gave NaN counts here (four steps: 1e-264), so a bound on four steps'
    shrink alone did not describe where it breaks; below the step-shrink bound
    it now rescales at every step."""
    run_estep(name, MU_NEAR, T)


def run_mlss(name, mu, T, check=True):
    c = case_of(name, mu)
    obs = sm.rare_obs(T, c.cards)
    path, logp, st = tgv.gpu_mlss(c.m, obs, c.ov, c.q)               # asserts last_kernel()
    seen("mlss", name, mu)
    if not check:
        return
    print("mlss %s mu=%g T=%d" % (name, mu, T))
    tgv.check(c.tables, c.cols(obs), path[:, :, 0], logp, st, c.N)


@pytest.mark.parametrize("mu,T", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("name", MLSS)
def test_mlss(name, mu, T):
    run_mlss(name, mu, T)


def run_stream(name, mu, T, L, check=True):
    c = case_of(name, mu)
    obs = sm.rare_obs(T, c.cards)
    if not check:
        tgs.stream_rows(c.m, c.ov, c.q, obs, L, [3, 4, T - 7])
        seen("stream", name, mu)
        return
    key = ("stream", name, mu, T, L)
    if key not in _refs:
        _refs[key] = su.fixed_lag(*c.tables, c.cols(obs), L)
    want, want_ll = _refs[key]
    rows, ll, st = tgs.stream_rows(c.m, c.ov, c.q, obs, L, [3, 4, T - 7])   # asserts last_kernel()
    seen("stream", name, mu)
    print("stream %s mu=%g T=%d L=%d" % (name, mu, T, L))
    tgs.check_rows(rows, want, tgs.ROW_TOL)
    tgs.check_ll(ll, want_ll)
    assert np.all(st == 0), st.tolist()


@pytest.mark.parametrize("L", [0, 3])
@pytest.mark.parametrize("mu,T", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("name", STREAMS)
def test_stream(name, mu, T, L):
    run_stream(name, mu, T, L)


def test_routes():
    """(operation, model, mu) -> kernel, one sweep at T = 24 (so the test
    stands alone), against the literal table: a routing change shows here."""
    for mu in sm.MUS:
        for name in SMOOTH:
            run_fb(name, mu, 24, False, check=False)
        for name in FILTER:
            run_fb(name, mu, 24, True, check=False)
        for name in ESTEP:
            run_estep(name, mu, 24, check=False)
        for name in MLSS:
            run_mlss(name, mu, 24, check=False)
        for name in STREAMS:
            run_stream(name, mu, 24, 3, check=False)
    for name in NEAR:
        run_estep(name, MU_NEAR, 24, check=False)
    got, want = {}, {}
    for (op, name, mu), ks in sorted(ROUTES.items()):
        got[(op, name, mu)] = " | ".join(sorted(ks))
        e = EXPECTED_NEAR.get(name) if mu == MU_NEAR else EXPECTED.get((op, name))
        want[(op, name, mu)] = e if isinstance(e, str) or e is None else e[sm.MUS.index(mu)]
    for key in sorted(got):
        print("route %-7s %-13s %-7g %s" % (key + (got[key],)))
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong
