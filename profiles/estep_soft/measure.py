"""The e_step under soft evidence against smoothing under the same evidence and
against the hard e_step, on hmm_spec(16, 16), M1 soft, B = 4096, T = 1024
("The e_step under soft evidence"): one process, every variant
warmed up, then 30 launches each, alternating, a pair of device events around
each launch; median, min..max.  Usage: python profiles/estep_soft/measure.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import nip_amd
from nip_amd import synth

B, T, N, M = 4096, 1024, 16, 16
nodes, pots = synth.hmm_spec(N, M)
m = nip_amd.Model.from_spec(nodes, pots)
P1, M1 = m.variable("P1"), m.variable("M1")
g = torch.Generator(device="cuda").manual_seed(1)
lik = 0.05 + torch.rand((B, T, M), dtype=torch.float64, device="cuda", generator=g)
obs = lik.argmax(dim=2, keepdim=True).to(torch.int32).contiguous()
post = torch.empty((B, T, N), dtype=torch.float64, device="cuda")
counts = torch.ones((m.param_size(),), dtype=torch.float64, device="cuda")
ll = torch.empty((B,), dtype=torch.float64, device="cuda")
st = torch.empty((B,), dtype=torch.int32, device="cuda")

calls = {
    "e_step_soft": lambda: nip_amd.e_step_soft(m, None, [], lik, [M1], counts=counts, ll=ll, status=st),
    "fb_soft": lambda: nip_amd.forward_backward_inference_soft(m, None, [], lik, [M1], [P1], post=post, ll=ll, status=st),
    "e_step_argmax": lambda: nip_amd.e_step(m, obs, [M1], counts=counts, ll=ll, status=st),
}
kern = {}
for k, f in calls.items():
    for _ in range(3):
        f()
    kern[k] = nip_amd.last_kernel()
torch.cuda.synchronize()
times = {k: [] for k in calls}
for rep in range(30):
    for k, f in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record()
        e1.synchronize()
        times[k].append(e0.elapsed_time(e1))
out = {k: {"kernel": kern[k], "median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
       for k, v in times.items()}
out["shape"] = {"B": B, "T": T, "N": N, "M": M}
# the weights twice and alpha^ out and back; fb_soft writes its rows besides
out["bytes_per_seq_step"] = {"e_step_soft": 8 * (2 * M + 2 * 16), "fb_soft": 8 * (2 * M + 3 * 16)}
for k, by in out["bytes_per_seq_step"].items():
    out[k]["tb_per_s"] = B * T * by / (out[k]["median_ms"] * 1e-3) / 1e12
out["e_step_soft_over_fb_soft"] = out["e_step_soft"]["median_ms"] / out["fb_soft"]["median_ms"]
out["e_step_soft_over_e_step_argmax"] = out["e_step_soft"]["median_ms"] / out["e_step_argmax"]["median_ms"]
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
