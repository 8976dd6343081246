"""The oracles of tests/test_gpu_small_mass.py pinned to each other on that
file's own inputs (small_mass_util: rare-symbol models, step masses down to
1e-150), so that a failure there cannot be the oracle's.  No GPU.

  PortOracle.fb          against textbook_util.smoother       (smoothed, filtered, ll)
  PortOracle.estep       against textbook_util.hmm_estep_torch (torch on the CPU)
  viterbi_util.viterbi   against viterbi_util.brute_force      (N = 3, T = 6)
  stream_util.fixed_lag  against the smoother on every prefix

Every one of these normalises at every step (the port oracle as the reference
does, nip.c:1461-1474), so the step's mass cancels before it can accumulate:
measured on these inputs, posteriors differ by at most 1.1e-16 and the ll by
1.3e-16 relative.  The bounds asserted are the project's (posteriors 1e-12,
ll 1e-12 relative, counts 1e-11 relative).  At s = 1e-250 the port oracle
itself gives up (-DBL_MAX): the matrix stops at 1e-150.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.bind import PortOracle

import small_mass_util as sm
import stream_util as su
import viterbi_util as vu
from em_util import close
from textbook_util import hmm_estep_torch, smoother

DBL_MAX = np.finfo(np.float64).max
T = 24


def build(kind, N, mu):
    if kind in ("hmm", "hmm-np"):
        return sm.rare_hmm(N, 4, sm.col_scale(mu, 1), proper=kind == "hmm")
    if kind == "demo":
        return sm.rare_demo(N, sm.col_scale(mu, 2))
    return sm.rare_star(N, sm.STAR_CARDS, sm.col_scale(mu, 4))


@pytest.mark.parametrize("mu", sm.MUS)
@pytest.mark.parametrize("kind,N", [("hmm", 16), ("hmm", 40), ("hmm-np", 16), ("demo", 20), ("star", 17)])
def test_port_oracle_fb_and_filter_vs_textbook(kind, N, mu):
    c = build(kind, N, mu)
    obs = sm.rare_obs(T, c.cards, B=8)
    A, pi, Es = c.tables
    post, filt, ll = smoother(A, pi, Es, c.cols(obs))
    assert np.isfinite(ll).all() and np.isfinite(post).all()
    orc = PortOracle(c.m.desc())
    worst = [0.0, 0.0, 0.0]
    for b in range(obs.shape[0]):
        rp, rl = orc.fb(obs[b], c.ov, c.q)
        fp, fl = orc.fb(obs[b], c.ov, c.q, filter_only=True)
        assert rl > -DBL_MAX and fl > -DBL_MAX
        worst[0] = max(worst[0], np.abs(rp - post[b]).max())
        worst[1] = max(worst[1], np.abs(fp - filt[b]).max())
        worst[2] = max(worst[2], abs(rl - ll[b]) / max(1.0, abs(ll[b])), abs(fl - ll[b]) / max(1.0, abs(ll[b])))
    print("smoothed %.3g filtered %.3g ll (relative) %.3g" % tuple(worst))
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12 and worst[2] <= 1e-12


@pytest.mark.parametrize("mu", sm.MUS)
@pytest.mark.parametrize("N,proper", [(16, True), (40, True), (16, False)])
def test_port_oracle_estep_vs_textbook(N, proper, mu):
    """The em_learn layout follows the declaration order (M1, P1, P0; or M1,
    P0, P1 with the transition normalised over P0); the textbook's is
    [P0 | P1|P0 | M1|P1]."""
    c = sm.rare_hmm(N, 4, mu, proper=proper)
    obs = sm.rare_obs(T, c.cards, B=8)
    A, pi, Es = c.tables
    M = Es[0].shape[1]
    want, wll = hmm_estep_torch(*(torch.from_numpy(np.ascontiguousarray(x)) for x in (A, pi, Es[0])),
                                torch.from_numpy(obs[:, :, 0]).long())
    want, wll = want.numpy(), wll.numpy()
    got, ll, bad = PortOracle(c.m.desc()).estep(obs, c.ov, np.zeros(c.m.param_size()))
    assert not bad.any()
    if proper:
        got = np.concatenate([got[M * N + N * N:], got[M * N:M * N + N * N], got[:M * N]])
    else:
        got = np.concatenate([got[M * N:M * N + N], got[M * N + N:], got[:M * N]])
    print("counts %.3g ll %.3g" % (np.abs(got - want).max(), np.abs(ll - wll).max()))
    assert close(got, want, 1e-11), np.abs(got - want).max()
    assert close(ll, wll, 1e-12)


def test_port_oracle_gives_up_below_the_matrix():
    """s = 1e-250: a run of rare steps leaves fp64 inside the port oracle's
    own propagation -- why the matrix stops at 1e-150."""
    c = sm.rare_hmm(16, 4, 1e-250)
    obs = sm.rare_obs(T, c.cards, B=5)
    orc = PortOracle(c.m.desc())
    assert any(orc.fb(obs[b], c.ov, c.q)[1] == -DBL_MAX for b in range(5))


@pytest.mark.parametrize("mu", sm.MUS)
def test_viterbi_vs_brute_force(mu):
    c = sm.rare_hmm(3, 4, mu)
    obs = sm.rare_obs(6, c.cards, B=8)
    A, pi, Es = c.tables
    path, logp = vu.viterbi(A, pi, Es, c.cols(obs))
    for b in range(obs.shape[0]):
        best, arg = vu.brute_force(A, pi, Es, [obs[b, :, 0]])
        assert abs(logp[b] - best) <= 1e-12 * max(1.0, abs(best)), (b, logp[b], best)
        score = vu.path_score(A, pi, Es, [obs[b:b + 1, :, 0]], path[b:b + 1])[0]
        assert abs(score - best) <= 1e-12 * max(1.0, abs(best))


@pytest.mark.parametrize("mu", sm.MUS)
@pytest.mark.parametrize("L", [0, 3])
def test_fixed_lag_vs_smoother_on_prefixes(L, mu):
    c = sm.rare_hmm(16, 4, mu)
    obs = sm.rare_obs(T, c.cards, B=8)
    A, pi, Es = c.tables
    cols = c.cols(obs)
    rows, ll = su.fixed_lag(A, pi, Es, cols, L)
    for t in range(T):
        end = min(t + L, T - 1) + 1
        post, _, pll = smoother(A, pi, Es, [x[:, :end] for x in cols])
        assert np.abs(rows[:, t] - post[:, t]).max() <= 1e-12
        if end == T:
            assert close(ll, pll, 1e-12)
