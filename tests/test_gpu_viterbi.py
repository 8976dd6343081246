"""most_likely_states / nipamd_mlss on the GPU (nip_amd/csrc/viterbi.hip,
chain_viterbi_kernel): the most likely sequence of the interface of a chain
plan, the reference's declared and never implemented mlss
(src/nip.h:431-438, src/nip.c:1620-1699).

There is no reference implementation; the oracle is the plain numpy Viterbi
of tests/viterbi_util.py over the model's own tables (pinned to its brute
force by tests/test_viterbi_api.py).  Per sequence:

 (a) every state is within its variable's cardinality;
 (b) the GPU path's own score (the sum of its log terms) is at least the
     oracle's optimum - 1e-11 max(1, |optimum|), and logp is within the same
     bound of the optimum (1e-11 relative: the project's ll tolerance,
     tests/test_gpu_fb_ckw.py);
 (c) at most 10 % of a batch's sequences have a path differing anywhere from
     the oracle's (near-ties at rounding level; each still passes (b)).

Shapes: B not a multiple of the sequences per wave (4, 2, 1) or per block, T
around the kernel's periods -- a back-pointer run is 16 steps at <= 16 states,
12 at 17..32, 10 at 33..64, and the path goes out 16 steps at a time.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import nip_amd
from nip_amd import synth

import viterbi_util as vu
from textbook_util import chain_tables

KERNEL = "chain_viterbi_kernel"
TOL = 1e-11


def gappy(B, T, cards, seed, frac=0.2):
    rng = np.random.default_rng(seed)
    obs = np.stack([rng.integers(0, c, size=(B, T)) for c in cards], axis=2).astype(np.int32)
    obs[rng.random(obs.shape) < frac] = -1
    return obs


def gpu_mlss(m, obs, ov, q):
    o = torch.from_numpy(np.ascontiguousarray(obs, np.int32)).cuda()
    path, logp, st = nip_amd.most_likely_states(m, o, ov, q)
    torch.cuda.synchronize()
    assert nip_amd.last_kernel() == KERNEL
    return path.cpu().numpy(), logp.cpu().numpy(), st.cpu().numpy()


def check(tables, cols, path, logp, st, N):
    """(a), (b), (c) for single-column paths [B, T] against the oracle; returns the oracle's path."""
    A, pi, Es = tables
    B, T = path.shape
    want, opt = vu.viterbi(A, pi, Es, cols, B=B, T=T)
    assert np.all(opt > -vu.DBL_MAX), "the case is meant to have mass everywhere"
    assert np.all(st == 0)
    assert path.min() >= 0 and path.max() < N                                       # (a)
    score = vu.path_score(A, pi, Es, cols, path.astype(np.int64))
    bound = TOL * np.maximum(1.0, np.abs(opt))
    print("max optimum - score %.3g, max |logp - optimum| %.3g (bound %.3g)"
          % ((opt - score).max(), np.abs(logp - opt).max(), bound.min()))
    assert np.all(score >= opt - bound), (opt - score).max()                        # (b)
    assert np.all(np.abs(logp - opt) <= bound), np.abs(logp - opt).max()
    differ = int((path != want).any(axis=1).sum())
    print("paths differing from the oracle's: %d / %d" % (differ, B))
    assert differ <= 0.10 * B, (differ, B)                                          # (c)
    return want


def hmm(N, M, seed, proper):
    nodes, pots = synth.hmm_spec(N, M, seed=seed, proper=proper)
    m = nip_amd.Model.from_spec(nodes, pots)
    P0, P1, M1 = m.variable("P0"), m.variable("P1"), m.variable("M1")
    return m, P1, M1, chain_tables(m, P0, P1, [M1])


@pytest.mark.parametrize("proper", [False, True])
@pytest.mark.parametrize("N,M,B,T", [(3, 4, 1, 1), (3, 4, 5, 2), (3, 4, 6, 3), (3, 4, 32, 67),
                                     (16, 16, 7, 5), (16, 16, 64, 300), (16, 16, 33, 129),
                                     (16, 16, 5, 15), (16, 16, 5, 16), (16, 16, 5, 17), (16, 16, 6, 33)])
def test_hmm_vs_oracle(N, M, B, T, proper):
    m, P1, M1, tables = hmm(N, M, 100 + N + T, proper)
    obs = gappy(B, T, (M,), 7 * B + T)
    path, logp, st = gpu_mlss(m, obs, [M1], [P1])
    check(tables, [obs[:, :, 0]], path[:, :, 0], logp, st, N)


def test_brute_force():
    """All 729 paths of every sequence: the GPU score is the enumerated maximum."""
    m, P1, M1, (A, pi, Es) = hmm(3, 4, 11, False)
    obs = gappy(8, 6, (4,), 3)
    path, logp, st = gpu_mlss(m, obs, [M1], [P1])
    score = vu.path_score(A, pi, Es, [obs[:, :, 0]], path[:, :, 0].astype(np.int64))
    for b in range(8):
        best, _ = vu.brute_force(A, pi, Es, [obs[b, :, 0]])
        assert abs(score[b] - best) <= TOL * max(1.0, abs(best))
        assert abs(logp[b] - best) <= TOL * max(1.0, abs(best))


def test_long_sequence_rescaling():
    """T = 4097: delta underflows after a few hundred steps unless the
    exponents are carried."""
    m, P1, M1, tables = hmm(16, 16, 21, True)
    obs = gappy(8, 4097, (16,), 5)
    path, logp, st = gpu_mlss(m, obs, [M1], [P1])
    assert np.all(logp < -4097.0)
    check(tables, [obs[:, :, 0]], path[:, :, 0], logp, st, 16)


def demo1(card, seed):
    nodes, pots = synth.demo1_spec(card, seed=seed)
    m = nip_amd.Model.from_spec(nodes, pots)
    v = {s: m.variable(s) for s in ("A1", "B1", "C0", "C1")}
    return m, v, chain_tables(m, v["C0"], v["C1"], [v["A1"], v["B1"]])


@pytest.mark.parametrize("card,B,T", [(20, 40, 203), (17, 9, 8), (32, 9, 8), (33, 9, 8),
                                      (20, 3, 11), (20, 3, 12), (20, 3, 13), (20, 5, 25),
                                      (33, 3, 9), (33, 3, 10), (33, 3, 11), (33, 2, 21)])
def test_wide_two_columns(card, B, T):
    m, v, tables = demo1(card, 300 + card)
    obs = gappy(B, T, (card, card), B + T)
    path, logp, st = gpu_mlss(m, obs, [v["A1"], v["B1"]], [v["C1"]])
    check(tables, [obs[:, :, 0], obs[:, :, 1]], path[:, :, 0], logp, st, card)


def test_wide_one_column_and_none():
    m, v, tables = demo1(20, 41)
    B, T = 40, 203
    obs = gappy(B, T, (20,), 9)
    none = np.full((B, T), -1)
    path, logp, st = gpu_mlss(m, obs, [v["B1"]], [v["C1"]])           # the second child's column only
    check(tables, [none, obs[:, :, 0]], path[:, :, 0], logp, st, 20)
    o = torch.empty((6, 19, 0), dtype=torch.int32, device="cuda")     # no evidence at all
    path, logp, st = nip_amd.most_likely_states(m, o, [], [v["C1"]])
    torch.cuda.synchronize()
    assert nip_amd.last_kernel() == KERNEL
    none = np.full((6, 19), -1)
    check(tables, [none, none], path.cpu().numpy()[:, :, 0], logp.cpu().numpy(), st.cpu().numpy(), 20)


def test_wide_gpu_fold():
    """config 5's shape: the transition folded on the GPU (64^4 in-clique)."""
    nodes, pots = synth.wide_spec(64, 8, seed=77)
    m = nip_amd.Model.from_spec(nodes, pots)
    X0, X1, O1 = m.variable("X0"), m.variable("X1"), m.variable("O1")
    obs = gappy(16, 130, (8,), 13)
    path, logp, st = gpu_mlss(m, obs, [O1], [X1])
    check(chain_tables(m, X0, X1, [O1]), [obs[:, :, 0]], path[:, :, 0], logp, st, 64)


def test_evidence_on_the_interface_variable():
    m, P1, M1, (A, pi, Es) = hmm(16, 16, 31, False)
    B, T = 9, 40
    rng = np.random.default_rng(8)
    obs = gappy(B, T, (16, 16), 17)
    seen = rng.random((B, T)) < 0.5
    obs[:, :, 1] = np.where(seen, rng.integers(0, 16, size=(B, T)), -1)
    path, logp, st = gpu_mlss(m, obs, [M1, P1], [P1])
    check((A, pi, Es + [np.eye(16)]), [obs[:, :, 0], obs[:, :, 1]], path[:, :, 0], logp, st, 16)
    assert np.array_equal(path[:, :, 0][seen], obs[:, :, 1][seen])


def test_exact_ties_take_the_lowest_state():
    """Dyadic uniform tables: every path ties exactly, and every product is
    exact, so the lowest-index rule alone decides -- all zeros.  (Declared
    child first, as synth.hmm_spec(proper=True), so that the compiled tables
    are the ones written here.)"""
    nodes = [("M1", 2, None), ("P1", 4, None), ("P0", 4, "P1")]
    pots = [("M1", ["P1"], np.full(8, 0.5)), ("P1", ["P0"], np.full(16, 0.25)), ("P0", [], np.full(4, 0.25))]
    m = nip_amd.Model.from_spec(nodes, pots)
    obs = gappy(6, 37, (2,), 2)
    path, logp, st = gpu_mlss(m, obs, [m.variable("M1")], [m.variable("P1")])
    assert np.all(st == 0)
    assert np.array_equal(path, np.zeros_like(path))
    n_seen = (obs[:, :, 0] >= 0).sum(axis=1)
    want = -(2.0 + 2.0 * 36 + n_seen) * np.log(2.0)          # u0 = 2^-2, 36 transitions 2^-2, 2^-1 per observation
    assert np.all(np.abs(logp - want) <= 1e-13 * np.abs(want))


def test_zero_mass_is_per_sequence():
    m, P1, M1, tables = hmm(3, 4, 51, False)
    obs = gappy(5, 23, (4,), 6)
    good = gpu_mlss(m, obs, [M1], [P1])
    bad = obs.copy()
    bad[2, 9, 0] = 4                                           # == M: out of range
    path, logp, st = gpu_mlss(m, bad, [M1], [P1])
    assert np.all(path[2] == -1) and logp[2] == -vu.DBL_MAX and st[2] & nip_amd.STATUS_ZERO_MASS
    keep = [0, 1, 3, 4]
    assert np.array_equal(path[keep], good[0][keep])
    assert np.array_equal(logp[keep], good[1][keep])
    assert np.all(st[keep] == 0)


def test_joint_interface():
    nodes, pots = synth.factorial_spec(4, 4, 5, seed=61)
    m = nip_amd.Model.from_spec(nodes, pots)
    d = m.desc()
    cur, prev = d["outgoing"], d["previous_outgoing"]
    X1, Y1, O1 = m.variable("X1"), m.variable("Y1"), m.variable("O1")
    A, pi, E = vu.joint_tables(m, prev, cur, O1)
    obs = gappy(12, 40, (5,), 19)
    path, logp, st = gpu_mlss(m, obs, [O1], [X1, Y1])
    assert path.shape == (12, 40, 2)
    assert path.min() >= 0 and path.max() < 4
    stride = {cur[0]: 1, cur[1]: m.card(cur[0])}
    joint = path[:, :, 0] * stride[X1] + path[:, :, 1] * stride[Y1]
    want = check((A, pi, [E]), [obs[:, :, 0]], joint, logp, st, 16)
    same = (joint == want).all(axis=1)
    assert np.array_equal(path[same, :, 0], (want[same] // stride[X1]) % 4)
    assert np.array_equal(path[same, :, 1], (want[same] // stride[Y1]) % 4)
    swapped, logp2, st2 = gpu_mlss(m, obs, [O1], [Y1, X1])
    assert np.array_equal(swapped[:, :, 0], path[:, :, 1]) and np.array_equal(swapped[:, :, 1], path[:, :, 0])
    assert np.array_equal(logp2, logp) and np.array_equal(st2, st)


def test_callers_buffers_and_stream():
    m, P1, M1, _ = hmm(16, 16, 71, False)
    obs = gappy(13, 50, (16,), 4)
    want = gpu_mlss(m, obs, [M1], [P1])
    o = torch.from_numpy(obs).cuda()
    path = torch.full((13, 50, 1), -7, dtype=torch.int32, device="cuda")
    logp = torch.zeros(13, dtype=torch.float64, device="cuda")
    st = torch.full((13,), 9, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = nip_amd.most_likely_states(m, o, [M1], [P1], path=path, logp=logp, status=st, stream=s)
    s.synchronize()
    assert got[0] is path and got[1] is logp and got[2] is st
    assert np.array_equal(path.cpu().numpy(), want[0])
    assert np.array_equal(logp.cpu().numpy(), want[1])
    assert np.array_equal(st.cpu().numpy(), want[2])
    with pytest.raises(nip_amd.NipError):
        nip_amd.most_likely_states(m, o, [M1], [P1], path=torch.zeros((13, 50, 1), device="cuda"))


def test_host_form_is_the_device_form():
    m, P1, M1, _ = hmm(3, 4, 81, True)
    obs = gappy(6, 21, (4,), 12)
    want = gpu_mlss(m, obs, [M1], [P1])
    path, logp, st = nip_amd.most_likely_states_host(m, obs, [M1], [P1])
    assert path.dtype == np.int32 and path.shape == (6, 21, 1)
    assert np.array_equal(path, want[0]) and np.array_equal(logp, want[1]) and np.array_equal(st, want[2])


def test_compat_mlss(tmp_path):
    """The reference's prototype through libnip.so: parse_model, read_timeseries, mlss(&P1, 1, ts)."""
    import test_compat as tc
    L = tc.load()
    L.mlss.restype = C.POINTER(tc.Series)
    L.mlss.argtypes = [C.POINTER(tc.VarP), C.c_int, C.POINTER(tc.Series)]
    src, _, _, _ = hmm(3, 4, 91, False)
    # write_model names, as the reference's does, the previous-slice variable in
    # the next-slice node's NIP_next, so one round trip swaps the two slices
    # and a second one restores the chain: the model under test is the twice
    # written one, for both APIs
    once, net = str(tmp_path / "once.net"), str(tmp_path / "hmm.net")
    nip_amd.write_model(src, once)
    nip_amd.write_model(nip_amd.Model.from_net(once), net)
    m = nip_amd.Model.from_net(net)
    P1, M1 = m.variable("P1"), m.variable("M1")
    names = m.state_names(M1)
    rng = np.random.default_rng(10)
    series = [[[rng.choice(names + ["null"])] for _ in range(T)] for T in (19, 1, 6)]
    data = str(tmp_path / "data.txt")
    tc.write_data(data, ["M1"], series)
    pm = L.parse_model(net.encode())
    assert pm
    ts = C.POINTER(C.POINTER(tc.Series))()
    assert L.read_timeseries(pm, data.encode(), C.byref(ts)) == 3
    L.nip_mark_variable(L.model_variable(pm, b"M1"))       # only marked columns are evidence (nip.c:982-1003)
    q = (tc.VarP * 1)(L.model_variable(pm, b"P1"))
    id0 = pm.contents.variables[0].contents.id
    for i, s in enumerate(series):
        obs = np.array([[names.index(r[0]) if r[0] != "null" else -1 for r in s]], np.int32)[:, :, None]
        want, _, st = nip_amd.most_likely_states_host(m, obs, [M1], [P1])
        assert st[0] == 0
        r = L.mlss(q, 1, ts[i])
        assert r
        rs = r.contents
        assert rs.length == len(s) and rs.num_of_observed == 1 and rs.num_of_hidden == m.num_vars - 1
        assert rs.observed[0].contents.id - id0 == P1
        assert [rs.hidden[k].contents.id - id0 for k in range(rs.num_of_hidden)] == \
               [v for v in range(m.num_vars) if v != P1]
        assert [rs.data[t][0] for t in range(rs.length)] == list(want[0, :, 0])
        L.free_timeseries(r)
    # outside the scope: NULL after the error handler took the code
    L.nip_reset_error_handler()
    bad = (tc.VarP * 1)(L.model_variable(pm, b"M1"))
    assert not L.mlss(bad, 1, ts[0])
    assert L.nip_check_error_type() == nip_amd.NIPAMD_ERROR_UNSUPPORTED
    L.nip_reset_error_handler()
    for i in range(3):
        L.free_timeseries(ts[i])
    L.free_model(pm)
