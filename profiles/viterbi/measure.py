#!/usr/bin/env python
"""Time nipamd_mlss (chain_viterbi_kernel) against nipamd_fb on the same
inputs, in one process: config 2 (N = M = 16, B = 4096, T = 1024) and config
4's shard (B = 131072, T = 1024).

Both entry points are warmed up until a second of launches has run.  A timed
window is a batch of --batch back-to-back launches of one entry point between
two device events (the launches queue faster than they run, so the host-side
call path is hidden behind the kernels; the figure is the window over the
batch size); --reps windows per entry point, the two entry points alternating,
median, min and max.  The bytes per sequence-step are the ones the algorithm
has to move, computed from the shapes: mlss reads the observation (4), writes
and re-reads its back-pointers (8 + 8 at N <= 16) and writes the path (4); fb
reads the observation and writes the posterior row (4 + 8 N), its scratch
traffic not counted.  The HBM fraction is those bytes over the time over the
peak bandwidth (8 TB/s).  Writes one JSON document (--out, default next to
this script) and prints it.  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

HBM_PEAK = 8.0e12
SHAPES = {"config2": (4096, 1024), "config4_shard": (131072, 1024)}


def warm(fn, torch):
    t0 = time.time()
    n = 0
    while n < 3 or time.time() - t0 < 1.0:               # code objects, tables, scratch, clocks
        fn()
        torch.cuda.synchronize()
        n += 1
    return n


def window(fn, batch, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def timed_pair(fns, reps, batch, torch):
    """fns: {name: callable}; windows alternate between the entry points."""
    warmups = {k: warm(f, torch) for k, f in fns.items()}
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ms[k].append(window(f, batch, torch))
    out = {}
    for k, v in ms.items():
        v = np.asarray(v)
        out[k] = {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()),
                  "reps": reps, "launches_per_window": batch, "warmup_launches": warmups[k]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--shapes", default="config2,config4_shard")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "measure.json"))
    args = ap.parse_args()
    import torch
    import nip_amd
    from nip_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing measured")
    N = M = 16
    nodes, pots = synth.hmm_spec(N, M, proper=True)
    m = nip_amd.Model.from_spec(nodes, pots)
    P1, M1 = m.variable("P1"), m.variable("M1")
    doc = {"device": torch.cuda.get_device_name(0), "N": N, "M": M, "hbm_peak_bytes_per_s": HBM_PEAK, "shapes": {}}
    for name in args.shapes.split(","):
        B, T = SHAPES[name]
        obs = torch.from_numpy(synth.observations(B, T, M, seed=7)).cuda()
        path = torch.empty((B, T, 1), dtype=torch.int32, device="cuda")
        logp = torch.empty(B, dtype=torch.float64, device="cuda")
        st = torch.empty(B, dtype=torch.int32, device="cuda")
        r = {"B": B, "T": T}
        post = torch.empty((B, T, N), dtype=torch.float64, device="cuda")
        ll = torch.empty(B, dtype=torch.float64, device="cuda")
        kernels = {}

        def run_mlss():
            nip_amd.most_likely_states(m, obs, [M1], [P1], path=path, logp=logp, status=st)
            kernels["mlss"] = nip_amd.last_kernel()

        def run_fb():
            nip_amd.forward_backward_inference(m, obs, [M1], [P1], post=post, ll=ll, status=st)
            kernels["fb"] = nip_amd.last_kernel()

        r.update(timed_pair({"mlss": run_mlss, "fb": run_fb}, args.reps, args.batch, torch))
        r["mlss"]["kernel"], r["fb"]["kernel"] = kernels["mlss"], kernels["fb"]
        r["mlss"]["bytes_per_seq_ts"] = 4 + 8 + 8 + 4
        r["fb"]["bytes_per_seq_ts"] = 4 + 8 * N
        for k in ("mlss", "fb"):
            s = r[k]["median_ms"] * 1e-3
            r[k]["seq_ts_per_s"] = B * T / s
            r[k]["hbm_fraction"] = r[k]["bytes_per_seq_ts"] * B * T / s / HBM_PEAK
        r["mlss_over_fb"] = r["mlss"]["median_ms"] / r["fb"]["median_ms"]
        doc["shapes"][name] = r
        del obs, path, post
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
