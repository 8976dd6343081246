"""Which kernel serves which request: one tiny request per host route, and the
name nip_amd.last_kernel() reports for it.

The host side of the hot path (csrc/engine_route.cpp, engine_fb.cpp,
engine_estep.cpp) chooses among some twenty kernels by the model's shape, the
evidence, the sequence length and the tables' values.  Numeric parity of each
kernel is the business of its own test file; this one pins the choice itself,
so that a change to the host code cannot silently move a request to another
kernel.  EXPECTED is a literal table: a row changes only together with a
deliberate change of the dispatch.

Shapes: B = 33 (two full 16-sequence groups and a ragged one), T = 9 (odd,
more than two chunks of four steps).  Every case asserts that ll is finite and
no status flag is set; the fb cases that each posterior row sums to 1 within
1e-12 (the named kernel ran and wrote the caller's views).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import nip_amd
from nip_amd import synth

pytestmark = pytest.mark.gpu

B, T = 33, 9
JT = "jt_filter_kernel + jt_post_kernel"

EXPECTED = {
    "fb_hmm16": "chain_fb_ckpt_kernel",
    "filter_hmm16": "chain_mfma_wide_kernel<1>",
    "fb_demo1_20": "chain_fb_ckw_kernel",
    "fb_demo1_20_peaked": "chain_mfma_wide_kernel<2>",
    "fb_demo1_40": "chain_row64_kernel",
    "fb_factorial": "chain_fb_ckpt_kernel<proj>",
    "fb_demo1_16_hidden_obs": "op_fb_kernel",
    "fb_demo1_16_hidden_obs_jtree": JT,
    "mlss_hmm16": "chain_viterbi_kernel",
    "estep_hmm16_proper": "chain_estep_ck_kernel",
    "estep_hmm16_peaked_proper": "chain_estep16_kernel",
    "estep_demo1_16": "chain_estep16_kernel",
    "estep_demo1_20": "chain_estep_ckw_kernel",
    "estep_demo1_20_peaked": "chain_estep_mw_kernel",
    "estep_demo1_40": JT,            # 84 count rows: beyond the wide chain e_step's slab (estep_wide_fits)
    "estep_hmm64": "chain_msgs_kernel + chain_stats_kernel",
    "estep_demo1_16_hidden_obs": "op_fb_kernel (e_step) + op_xi_sort_kernel",
    "estep_demo1_16_hidden_obs_plain_partial":
        JT + " (general engine: an operator-chain request on a partial without room for its section)",
}


def _near_identity(n, eps):
    d = np.full((n, n), eps)
    np.fill_diagonal(d, 1.0)
    return (d / d.sum(axis=1, keepdims=True)).ravel()


def _hmm(proper=False, N=16):
    nodes, pots = synth.hmm_spec(N, 16, proper=proper)
    return nip_amd.Model.from_spec(nodes, pots), ["M1"], ["P1"]


def _peaked_hmm():
    """the model of test_gpu_estep.py test_estep_peaked_proper_model_sparse_rescaling"""
    N = 16
    nodes = [("P0", N, "P1"), ("P1", N, None), ("M1", N, None)]
    pots = [("M1", ["P1"], _near_identity(N, 1e-60)),
            ("P1", ["P0"], _near_identity(N, 1e-50)),
            ("P0", [], np.full(N, 1.0 / N))]
    return nip_amd.Model.from_spec(nodes, pots), ["M1"], ["P1"]


def _demo1(card, peaked=False, hidden_obs=False):
    nodes, pots = synth.demo1_spec(card)
    if peaked:                       # (A1 | C1) near the identity: step_shrink_ok's bound fails
        name, par, _ = pots[0]
        pots = [(name, par, _near_identity(card, 1e-50))] + list(pots[1:])
    return (nip_amd.Model.from_spec(nodes, pots), ["A1", "B1"] + (["D1"] if hidden_obs else []), ["C1"])


def _factorial():
    nodes, pots = synth.factorial_spec(4, 3, 5)
    return nip_amd.Model.from_spec(nodes, pots), ["O1"], ["X1", "Y1"]


# name -> (operation, model builder, engine)
CASES = {
    "fb_hmm16": ("fb", _hmm, nip_amd.ENGINE_AUTO),
    "filter_hmm16": ("filter", _hmm, nip_amd.ENGINE_AUTO),
    "fb_demo1_20": ("fb", lambda: _demo1(20), nip_amd.ENGINE_AUTO),
    "fb_demo1_20_peaked": ("fb", lambda: _demo1(20, peaked=True), nip_amd.ENGINE_AUTO),
    "fb_demo1_40": ("fb", lambda: _demo1(40), nip_amd.ENGINE_AUTO),
    "fb_factorial": ("fb", _factorial, nip_amd.ENGINE_AUTO),
    "fb_demo1_16_hidden_obs": ("fb", lambda: _demo1(16, hidden_obs=True), nip_amd.ENGINE_AUTO),
    "fb_demo1_16_hidden_obs_jtree": ("fb", lambda: _demo1(16, hidden_obs=True), nip_amd.ENGINE_JTREE),
    "mlss_hmm16": ("mlss", _hmm, nip_amd.ENGINE_AUTO),
    "estep_hmm16_proper": ("estep", lambda: _hmm(proper=True), nip_amd.ENGINE_AUTO),
    "estep_hmm16_peaked_proper": ("estep", _peaked_hmm, nip_amd.ENGINE_AUTO),
    "estep_demo1_16": ("estep", lambda: _demo1(16), nip_amd.ENGINE_AUTO),
    "estep_demo1_20": ("estep", lambda: _demo1(20), nip_amd.ENGINE_AUTO),
    "estep_demo1_20_peaked": ("estep", lambda: _demo1(20, peaked=True), nip_amd.ENGINE_AUTO),
    "estep_demo1_40": ("estep", lambda: _demo1(40), nip_amd.ENGINE_AUTO),
    "estep_hmm64": ("estep", lambda: _hmm(N=64), nip_amd.ENGINE_AUTO),
    "estep_demo1_16_hidden_obs": ("estep", lambda: _demo1(16, hidden_obs=True), nip_amd.ENGINE_AUTO),
    "estep_demo1_16_hidden_obs_plain_partial":
        ("plain_partial", lambda: _demo1(16, hidden_obs=True), nip_amd.ENGINE_AUTO),
}


def _plain_partial(m, obs, ov):
    """nipamd_estep_partial: no capacity argument, nipamd_estep_partial_size doubles"""
    L = nip_amd.lib()
    part = torch.zeros(L.nipamd_estep_partial_size(m._h), dtype=torch.float64, device="cuda")
    ll = torch.empty(obs.shape[0], dtype=torch.float64, device="cuda")
    st = torch.empty(obs.shape[0], dtype=torch.int32, device="cuda")
    rc = L.nipamd_estep_partial(m._h, C.c_void_p(obs.data_ptr()), len(ov), (C.c_int * len(ov))(*ov),
                                obs.shape[0], obs.shape[1], C.c_void_p(part.data_ptr()),
                                C.c_void_p(ll.data_ptr()), C.c_void_p(st.data_ptr()), None)
    assert rc == 0, nip_amd.lib().nipamd_last_error()
    return part, ll, st


def run_case(name):
    """The case's request once: {"kernel", "out" (posteriors / path / counts /
    partial), "ll", "status"} as host values."""
    op, build, engine = CASES[name]
    m, ov, q = build()
    ov, q = [m.variable(s) for s in ov], [m.variable(s) for s in q]
    cols = [synth.observations(B, T, m.card(v), seed=7 + i)[:, :, 0] for i, v in enumerate(ov)]
    obs = torch.from_numpy(np.ascontiguousarray(np.stack(cols, axis=2))).cuda()
    m.set_engine(engine)
    if op == "fb":
        out, ll, st = nip_amd.forward_backward_inference(m, obs, ov, q)
    elif op == "filter":
        out, ll, st = nip_amd.forward_inference(m, obs, ov, q)
    elif op == "mlss":
        out, ll, st = nip_amd.most_likely_states(m, obs, ov, q)
    elif op == "estep":
        out, ll, st = nip_amd.e_step(m, obs, ov)
    else:
        out, ll, st = _plain_partial(m, obs, ov)
    torch.cuda.synchronize()
    kernel = nip_amd.last_kernel()
    return {"op": op, "kernel": kernel, "out": out.cpu().numpy(), "ll": ll.cpu().numpy(),
            "status": st.cpu().numpy(), "cards": [m.card(v) for v in q]}


@pytest.mark.parametrize("name", list(CASES))
def test_request_runs_on_its_kernel(name):
    r = run_case(name)
    print(name, "->", r["kernel"])
    assert r["kernel"] == EXPECTED[name], r["kernel"]
    assert np.isfinite(r["ll"]).all()
    assert not r["status"].any()
    assert np.isfinite(r["out"].astype(np.float64)).all()
    if r["op"] in ("fb", "filter"):
        off = 0
        for card in r["cards"]:
            s = r["out"][:, :, off:off + card].sum(axis=2)
            print(name, "largest |row sum - 1|", np.abs(s - 1.0).max())
            assert np.abs(s - 1.0).max() <= 1e-12
            off += card
