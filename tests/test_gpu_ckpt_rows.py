"""Row-form phase A of the checkpoint kernel (chain_ckpt.hip, RowsA) and its
hand-over to the matrix-core phase B.

Phase A runs H = T / 2 forward and T - 1 - H backward steps in 16-lane rows,
grouped by four from the checkpoint steps, and hands the filters' next input,
the pending scale and the forward ll state to phase B through LDS.  The cases
sit on the edges of that: phases of 0 to 6 steps (no checkpoint, exactly one,
no group at all), short last blocks, sequences that die on either side of the
hand-over, missing runs over a whole phase, and a near-identity model whose
step mass (about 1e-29) sits just above the step-shrink bound of the kernels
that rescale every 4th step (engine_route.cpp): it takes this kernel, and a
group of four steps shrinks a row to about 1e-116 between rescales, so the
row-form rescaling, the checkpoint scaling and the ll exponents all matter.
(_fb_worker's peaked 1e-50 / 1e-60 model lies below that bound and is routed
to chain_mfma_wide_kernel, which rescales every step: its cases here check
that route's results only.)  Every other case asserts that the checkpoint
kernel ran.  All are checked against the oracle (posteriors 1e-12, ll 1e-12
relative, status).  One case compares every
tests/_fb_worker.py case with the matrix-core phase A, which the diagnostics
library runs with NIPAMD_CK_PHASEA=mfma (csrc/diag.h): posteriors 4e-16, ll
1e-14 relative, status equal, as tests/test_gpu_ckpt.py compares the two
16-state kernels; the two phase-A forms round differently, so a difference
of exactly zero everywhere would mean the switch did not take effect.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import nip_amd
from nip_amd import synth
from oracle.bind import PortOracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fb_worker  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DBL_MAX = np.finfo(np.float64).max
INVALID = 16


def plain_model(seed):
    nodes, pots = synth.hmm_spec(16, 16, seed=seed)       # as _fb_worker.build_case
    return nip_amd.Model.from_spec(nodes, pots)


def near_bound_model(eps_emit=1e-29, eps_trans=1e-40):
    """Near-identity 16-state HMM: a step costs a mismatched observation
    (eps_emit) rather than a state change (eps_trans), so every step's mass is
    about eps_emit and step_shrink is eps_emit / (1 + 15 eps_emit) >= 1e-30."""
    N = 16
    nodes = [("P0", N, "P1"), ("P1", N, None), ("M1", N, None)]
    pots = [("M1", ["P1"], _fb_worker.near_identity(N, eps_emit)),
            ("P1", ["P0"], _fb_worker.near_identity(N, eps_trans)),
            ("P0", [], np.full(N, 1.0 / N))]
    return nip_amd.Model.from_spec(nodes, pots)


def check_oracle(m, obs, kernel="chain_fb_ckpt_kernel"):
    ov, q = [m.variable("M1")], [m.variable("P1")]
    post, ll, st = _fb_worker.run(m, obs, ov, q)
    if kernel:
        assert nip_amd.last_kernel() == kernel, nip_amd.last_kernel()
    orc = PortOracle(m.desc())
    for b in range(obs.shape[0]):
        rp, rl = orc.fb(obs[b], ov, q)
        assert np.abs(post[b] - rp).max() <= 1e-12, (b, np.abs(post[b] - rp).max())
        if rl == -DBL_MAX:
            assert ll[b] == -DBL_MAX, (b, ll[b])
        else:
            assert abs(ll[b] - rl) <= 1e-12 * max(1.0, abs(rl)), (b, ll[b], rl)
        assert st[b] == (1 if rl == -DBL_MAX else 0), (b, st[b], rl)
    return ll


@pytest.mark.parametrize("T", [2, 3, 4, 5, 7, 8, 9, 12, 13])
def test_short_phase_a(T):
    check_oracle(plain_model(200 + T), synth.observations(5, T, 16, seed=900 + T))


@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_short_last_block(B):
    check_oracle(plain_model(300 + B), synth.observations(B, 21, 16, seed=950 + B))


@pytest.mark.parametrize("where", ["t0", "H-1", "H", "T-1"])
def test_invalid_code_around_hand_over(where):
    T, B = 40, 5
    H = T // 2
    t = {"t0": 0, "H-1": H - 1, "H": H, "T-1": T - 1}[where]
    obs = synth.observations(B, T, 16, seed=77)
    obs[1, t, 0] = INVALID
    obs[3, t, 0] = INVALID
    ll = check_oracle(plain_model(41), obs)
    assert ll[1] == -DBL_MAX and ll[3] == -DBL_MAX and np.all(ll[[0, 2, 4]] > -DBL_MAX)


@pytest.mark.parametrize("first_half_missing", [True, False])
def test_missing_run_over_a_phase(first_half_missing):
    T, B = 40, 5
    H = T // 2
    obs = synth.observations(B, T, 16, seed=78)
    if first_half_missing:
        obs[:, :H, 0] = -1          # the forward rows' whole phase A
    else:
        obs[:, H:, 0] = -1          # the backward rows' whole phase A
    check_oracle(plain_model(42), obs)


@pytest.mark.parametrize("T", [9, 40])
def test_peaked_model_rows(T):
    # below the step-shrink bound: routed away from the checkpoint kernel (see the module docstring)
    m = _fb_worker.build_case("peaked")[0]
    check_oracle(m, synth.observations(7, T, 16, seed=500 + T), kernel=None)
    assert nip_amd.last_kernel() != "chain_fb_ckpt_kernel"


# T = 53: H = 26 forward steps (a 2-step prelude, six groups), 26 backward (2 + six groups)
@pytest.mark.parametrize("T", [9, 40, 53])
def test_near_bound_model_rows(T):
    ll = check_oracle(near_bound_model(), synth.observations(7, T, 16, seed=600 + T))
    assert np.all(ll < -30.0 * T)          # most steps do cost about 1e-29: the rescaling is exercised


def test_rows_vs_matrix_core_phase_a():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "mfma_a.npz")
        from nip_amd import build as nb
        env = dict(os.environ, NIPAMD_CK_PHASEA="mfma", NIPAMD_LIB=nb.DIAG_LIB)   # a diagnostics-build switch
        r = subprocess.run([sys.executable, os.path.join(HERE, "_fb_worker.py"), out], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        with np.load(out) as z:
            ref = {k: z[k] for k in z.files}
    worst = 0.0
    for name in _fb_worker.CASES:
        post, ll, st = _fb_worker.run(*_fb_worker.build_case(name))
        dp = np.abs(ref[name + "/post"] - post).max()
        dl = (np.abs(ref[name + "/ll"] - ll) / np.maximum(1.0, np.abs(ll))).max()
        print("%-14s posteriors %.3g  ll %.3g" % (name, dp, dl))
        assert dp <= 4e-16, name
        assert dl <= 1e-14, name
        assert np.array_equal(ref[name + "/st"], st), name
        worst = max(worst, dp, dl)
    assert worst > 0.0, "NIPAMD_CK_PHASEA=mfma did not select another phase A"
