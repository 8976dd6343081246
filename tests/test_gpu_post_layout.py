"""Every forward_backward_inference / forward_inference route writes exactly
its own rows: the caller's post, ll and status are views inside larger device
allocations filled with a sentinel, and after the call the guard words on
either side are untouched, every word inside was written, and the values are
the CPU oracle's (pinned to the reference by tests/test_oracle.py).

What the kernels are not told by one-cardinality models: the row of a query
is as wide as its variables add up to, the interface variable's marginals
start at any offset in it, and the buffer starts at any 8-byte boundary.
Several kernels store 16 bytes at a time where rows are as wide as their
padded state count (16, 32, 64) and aligned; the conditions for that are the
ones under test (chain_ckpt.hip, chain_mfma.hip, chain_mfma_wide.hip,
estep_ckw.hip chain_fb_ckw_kernel, whose condition missed N == 32: a 2-state
child queried before a 30-state interface made every step write 32 doubles
from offset 2, two of them past its row and at last past the buffer).

Models with mixed cardinalities (synth builders with unequal arguments, the
demo1 structure inline), so a child's width plus the interface's reaches the
padded row with an even and an odd offset.  B = 17 (two 16-sequence groups,
one live sequence in the last), T = 1, 4, 5, 7 (every T mod 4 and the
checkpoint kernels' chunk tails), 15 % of the observations missing.
Tolerances as test_gpu_fb_ckw.py: posteriors 1e-12 absolute, ll 1e-11
relative.  The last test pins the routes the file went through.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import nip_amd
from nip_amd import synth
from oracle.bind import PortOracle

DBL_MAX = np.finfo(np.float64).max
B = 17
TS = (1, 4, 5, 7)
GUARDS = (64, 65)                     # the view starts on a 16-byte boundary / 8 bytes off one
SENT64 = 0x4B1D5EEDC0FFEE11           # as a double: 1.6e55, finite; no posterior, ll or status word looks like it
SENT32 = 0x5EEDC0DE
PTOL, LTOL = 1e-12, 1e-11

FBCK = "chain_fb_ckw_kernel"
MW1, MW2 = "chain_mfma_wide_kernel<1>", "chain_mfma_wide_kernel<2>"
CKPT, PROJ, MFMA = "chain_fb_ckpt_kernel", "chain_fb_ckpt_kernel<proj>", "chain_fb_mfma_kernel"
ROW64 = "chain_row64_kernel"
OP, OPW = "op_fb_kernel", "op_wide_msgs_kernel + op_wide_post_kernel"
JT = "jt_filter_kernel + jt_post_kernel"

SEEN = set()                          # (operation, kernel) of every request of this file


def demo1_mixed(a, c, peaked=False, b=3, d=2, seed=7):
    """The demo1 structure with a small A1 (a states), B1 (b), D1 (d) and a
    c-state interface C0 -> C1.  peaked: B1 emits (nearly) only state C1 mod b,
    1e-40 elsewhere, which fails the host's bound for rescaling every 4th
    step (step_shrink_ok) and keeps the request on chain_mfma_wide_kernel."""
    if peaked:
        e = np.full((c, b), 1e-40)
        e[np.arange(c), np.arange(c) % b] = 1.0
        e = (e / e.sum(axis=1, keepdims=True)).ravel()
    else:
        e = synth.cpt(seed + 1, b, c)
    nodes = [("A1", a, None), ("B1", b, None), ("C0", c, "C1"), ("C1", c, None), ("D1", d, None)]
    pots = [("A1", ["C1"], synth.cpt(seed, a, c)),
            ("B1", ["C1"], e),
            ("C0", [], synth.cpt(seed + 2, c, 1)),
            ("D1", [], synth.cpt(seed + 3, d, 1)),
            ("C1", ["D1", "C0"], synth.cpt(seed + 4, c, d * c))]
    return nodes, pots


def hmm(N, M):
    return lambda: synth.hmm_spec(N, M, seed=100 + N)


HMM_LAYOUTS = (["P1"], ["M1", "P1"], ["P1", "M1"], ["P1", "M1", "P1"])
DEMO_LAYOUTS = (["C1"], ["A1", "C1"], ["C1", "A1"], ["C1", "A1", "C1"])

# name -> (spec, observed, query layouts, engine, kernels smoothing may run on, kernels filtering may)
CASES = {
    # one observed column, 17..32 states: chain_fb_ckw_kernel; filtering on chain_mfma_wide_kernel<2>.
    # 2 + 30 and 3 + 29 fill the 32-wide row from an even and an odd offset; 32 alone takes the 16-byte stores
    "hmm30x2": (hmm(30, 2), ["M1"], HMM_LAYOUTS, nip_amd.ENGINE_AUTO, (FBCK,), (MW2,)),
    "hmm29x3": (hmm(29, 3), ["M1"], HMM_LAYOUTS, nip_amd.ENGINE_AUTO, (FBCK,), (MW2,)),
    "hmm32x2": (hmm(32, 2), ["M1"], HMM_LAYOUTS, nip_amd.ENGINE_AUTO, (FBCK,), (MW2,)),
    # one observed column, up to 16 states: chain_fb_ckpt_kernel where the rows are 16 wide and aligned (16
    # states), chain_fb_mfma_kernel otherwise (and at T = 1); filtering on chain_mfma_wide_kernel<1>
    "hmm14x2": (hmm(14, 2), ["M1"], HMM_LAYOUTS, nip_amd.ENGINE_AUTO, (MFMA,), (MW1,)),
    "hmm13x3": (hmm(13, 3), ["M1"], HMM_LAYOUTS, nip_amd.ENGINE_AUTO, (MFMA,), (MW1,)),
    "hmm16x2": (hmm(16, 2), ["M1"], HMM_LAYOUTS, nip_amd.ENGINE_AUTO, (CKPT, MFMA), (MW1,)),
    # two observed columns: chain_fb_ckw_kernel at 17..32 states, chain_mfma_wide_kernel<1> up to 16
    "demo30": (lambda: demo1_mixed(2, 30), ["A1", "B1"], DEMO_LAYOUTS, nip_amd.ENGINE_AUTO, (FBCK,), (MW2,)),
    "demo29": (lambda: demo1_mixed(3, 29), ["A1", "B1"], DEMO_LAYOUTS, nip_amd.ENGINE_AUTO, (FBCK,), (MW2,)),
    "demo14": (lambda: demo1_mixed(2, 14), ["A1", "B1"], DEMO_LAYOUTS, nip_amd.ENGINE_AUTO, (MW1,), (MW1,)),
    "demo13": (lambda: demo1_mixed(3, 13), ["A1", "B1"], DEMO_LAYOUTS, nip_amd.ENGINE_AUTO, (MW1,), (MW1,)),
    "demo16": (lambda: demo1_mixed(2, 16), ["A1", "B1"], DEMO_LAYOUTS, nip_amd.ENGINE_AUTO, (MW1,), (MW1,)),
    # the rescaling bound fails: smoothing on chain_mfma_wide_kernel<2>
    "demo30_peaked": (lambda: demo1_mixed(2, 30, peaked=True), ["A1", "B1"], DEMO_LAYOUTS, nip_amd.ENGINE_AUTO,
                      (MW2,), (MW2,)),
    "demo29_peaked": (lambda: demo1_mixed(3, 29, peaked=True), ["A1", "B1"], DEMO_LAYOUTS, nip_amd.ENGINE_AUTO,
                      (MW2,), (MW2,)),
    "demo32_peaked": (lambda: demo1_mixed(2, 32, peaked=True), ["A1", "B1"], DEMO_LAYOUTS, nip_amd.ENGINE_AUTO,
                      (MW2,), (MW2,)),
    # 33..64 states: chain_row64_kernel; 2 + 62 and 3 + 61 fill the 64-wide row
    "hmm62x2": (hmm(62, 2), ["M1"], HMM_LAYOUTS, nip_amd.ENGINE_AUTO, (ROW64,), (ROW64,)),
    "hmm61x3": (hmm(61, 3), ["M1"], HMM_LAYOUTS, nip_amd.ENGINE_AUTO, (ROW64,), (ROW64,)),
    "hmm64x2": (hmm(64, 2), ["M1"], HMM_LAYOUTS, nip_amd.ENGINE_AUTO, (ROW64,), (ROW64,)),
    # a joint interface of 16 states: chain_fb_ckpt_kernel's projections when every query is one of its
    # variables, the joint marginal and derive_kernel's projections otherwise (O1: a leaf child; filtering)
    "factorial445": (lambda: synth.factorial_spec(4, 4, 5), ["O1"],
                     (["X1"], ["Y1", "X1"], ["X1", "Y1"], ["X1", "Y1", "X1"], ["O1", "X1"]),
                     nip_amd.ENGINE_AUTO, (PROJ, CKPT, MFMA), (MW1,)),
    # the general join-tree engine
    "factorial435_jtree": (lambda: synth.factorial_spec(4, 3, 5), ["O1"],
                           (["X1"], ["Y1", "X1"], ["X1", "O1"], ["X1", "Y1", "X1"]),
                           nip_amd.ENGINE_JTREE, (JT,), (JT,)),
    # evidence on a non-leaf variable (O1 has the observed child Q1): the operator chain, which writes a
    # single interface query straight into its rows and projects several out of its work buffer (a query off
    # the interface sends the request on to the general engine)
    "nonleaf5": (lambda: synth.nonleaf_spec(5, 3, 3), ["O1", "Q1"],
                 (["P1"], ["P1", "P1"], ["P1", "P1", "P1"], ["Q1", "P1"], ["P1", "O1"]),
                 nip_amd.ENGINE_AUTO, (OP, JT), (OP, JT)),
    # evidence on the hidden parent D1 at 21 interface states: the operator chain's wide kernels
    "demo21_D1": (lambda: demo1_mixed(2, 21), ["A1", "B1", "D1"], (["C1"], ["C1", "C1"], ["A1", "C1"]),
                  nip_amd.ENGINE_AUTO, (OPW, JT), (OPW, JT)),
}
# the folded in-clique of wide_spec (33^4 entries: the oracle takes a third of a second per sequence, so one
# smoothing request; the 64-wide rows are the HMM shapes' above)
WIDE_CASE = ("wide33", lambda: synth.wide_spec(33, 2), ["O1"], ["O1", "X1"], 5)

_models, _refs = {}, {}


def model_of(name):
    if name not in _models:
        spec = WIDE_CASE[1] if name == WIDE_CASE[0] else CASES[name][0]
        engine = nip_amd.ENGINE_AUTO if name == WIDE_CASE[0] else CASES[name][3]
        m = nip_amd.Model.from_spec(*spec())
        m.set_engine(engine)
        _models[name] = (m, PortOracle(m.desc()))
    return _models[name]


def gappy(T, cards, seed, frac=0.15):
    rng = np.random.default_rng(seed)
    obs = np.stack([rng.integers(0, c, size=(B, T)) for c in cards], axis=2).astype(np.int32)
    obs[rng.random(obs.shape) < frac] = -1
    return obs


def reference(name, T, osyms, qsyms, filt):
    """(obs, ov, q, posteriors [B][T][width], ll [B]) of the oracle, computed
    once per request and shared by the guard offsets."""
    key = (name, T, tuple(qsyms), filt)
    if key not in _refs:
        m, orc = model_of(name)
        ov, q = [m.variable(s) for s in osyms], [m.variable(s) for s in qsyms]
        obs = gappy(T, [m.card(v) for v in ov], 1000 * T + len(name))
        if filt:
            out = [orc.fb(obs[b], ov, q, filter_only=True) for b in range(B)]
            rp, rl = np.stack([o[0] for o in out]), np.array([o[1] for o in out])
        else:
            rp, rl = orc.fb_batch(obs, ov, q, nthreads=8)      # no_fb per sequence, as PortOracle.fb
        _refs[key] = (obs, ov, q, rp, rl)
    return _refs[key]


def guarded(n, guard, dtype):
    """(whole allocation as integers, the n-element view `guard` elements in):
    guard + n + guard elements, every word the sentinel."""
    if dtype == torch.float64:
        raw = torch.full((guard + n + guard,), SENT64, dtype=torch.int64, device="cuda")
    else:
        raw = torch.full((guard + n + guard,), SENT32, dtype=torch.int32, device="cuda")
    return raw, raw.view(dtype)[guard:guard + n]


def check_guarded(name, T, osyms, qsyms, guard, filt, allowed):
    """The request into caller-owned views between guards: (a) the guards keep
    the sentinel, (b) no word inside does, (c) the values are the oracle's.
    Returns the kernel."""
    m, _ = model_of(name)
    obs, ov, q, rp, rl = reference(name, T, osyms, qsyms, filt)
    width = rp.shape[2]
    raws, views = {}, {}
    for what, n, dt in (("post", B * T * width, torch.float64), ("ll", B, torch.float64), ("status", B, torch.int32)):
        raws[what], views[what] = guarded(n, guard, dt)
    post = views["post"].view(B, T, width)
    assert post.is_contiguous() and post.data_ptr() % 16 == 8 * (guard & 1)
    fn = nip_amd.forward_inference if filt else nip_amd.forward_backward_inference
    o = torch.from_numpy(obs).cuda()
    fn(m, o, ov, q, post=post, ll=views["ll"], status=views["status"])
    torch.cuda.synchronize()
    kernel = nip_amd.last_kernel()
    SEEN.add(("filter" if filt else "fb", kernel))
    where = "%s T=%d %s guard=%d %s on %s" % (name, T, "+".join(qsyms), guard, "filter" if filt else "fb", kernel)
    for what, raw in raws.items():
        sent = SENT32 if what == "status" else SENT64
        r = raw.cpu().numpy()
        n = r.size - 2 * guard
        lo, hi, body = r[:guard], r[guard + n:], r[guard:guard + n]
        assert (lo == sent).all(), "%s: %s written before its start, words %s" % (where, what, np.nonzero(lo != sent)[0] - guard)
        assert (hi == sent).all(), "%s: %s written past its end, words +%s" % (where, what, np.nonzero(hi != sent)[0])
        assert (body != sent).all(), "%s: %d words of %s never written" % (where, int((body == sent).sum()), what)
    assert kernel in allowed, where
    gp, gl, gs = post.cpu().numpy(), views["ll"].cpu().numpy(), views["status"].cpu().numpy()
    for b in range(B):
        if rl[b] == -DBL_MAX:
            assert gl[b] == -DBL_MAX and gs[b], (where, b)
            continue
        err = np.abs(gp[b] - rp[b]).max()
        assert err <= PTOL, "%s: sequence %d: posterior error %g" % (where, b, err)
        assert abs(gl[b] - rl[b]) <= LTOL * max(1.0, abs(rl[b])), (where, b, gl[b], rl[b])
        assert gs[b] == 0, (where, b)
    return kernel


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", list(CASES))
def test_smoothing_writes_exactly_its_rows(name, T):
    _, osyms, layouts, _, allowed, _ = CASES[name]
    for qsyms in layouts:
        for guard in GUARDS:
            check_guarded(name, T, osyms, qsyms, guard, False, allowed)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", list(CASES))
def test_filtering_writes_exactly_its_rows(name, T):
    _, osyms, layouts, _, _, allowed = CASES[name]
    for qsyms in layouts:
        for guard in GUARDS:
            check_guarded(name, T, osyms, qsyms, guard, True, allowed)


@pytest.mark.parametrize("guard", GUARDS)
@pytest.mark.parametrize("T", TS)
def test_binary_child_before_a_30_state_interface_on_the_ckw_kernel(T, guard):
    """[2-state child, 30-state interface], one observed column, smoothing:
    row stride 32, interface offset 2, on chain_fb_ckw_kernel itself.  With
    16-byte stores taken on the stride alone, each step wrote 32 doubles from
    offset 2: the last row's tail landed in the first two guard words."""
    k = check_guarded("hmm30x2", T, ["M1"], ["M1", "P1"], guard, False, (FBCK,))
    assert k == FBCK


def test_folded_in_clique_at_33_states_writes_exactly_its_rows():
    """wide_spec's in-clique (X0, Y1, Z1, X1) folded on the GPU, 33 states:
    [2-state child, interface], an odd row of 35 doubles, T odd."""
    name, _, osyms, qsyms, T = WIDE_CASE
    for guard in GUARDS:
        check_guarded(name, T, osyms, qsyms, guard, False, (ROW64,))


def test_every_route_was_taken():
    """The union of (operation, kernel) over this file's requests (one more
    sweep here, so the test stands alone): the seven routes and each width
    class's filter kernel, by the names nip_amd.last_kernel() reports."""
    for name, (_, osyms, layouts, _, fb_k, fi_k) in CASES.items():
        for guard in GUARDS:
            check_guarded(name, 5, osyms, layouts[0], guard, False, fb_k)
            check_guarded(name, 5, osyms, layouts[0], guard, True, fi_k)
    print(sorted(SEEN))
    want = {("fb", FBCK), ("fb", MW1), ("fb", MW2), ("fb", CKPT), ("fb", PROJ), ("fb", MFMA), ("fb", ROW64),
            ("filter", MW1), ("filter", MW2), ("filter", ROW64),
            ("fb", OP), ("filter", OP), ("fb", OPW), ("filter", OPW), ("fb", JT), ("filter", JT)}
    assert want <= SEEN, sorted(want - SEEN)
