#!/usr/bin/env python
"""Time online inference under soft evidence (nip_amd.Stream with soft_vars,
chain_stream_soft_kernel) in one process: hmm_spec(16, 16) with M1 soft,
B = 4096 and 131072, 1024 steps per pass.

Variants of a pass (a reset, then 1024 steps pushed; rows go to one reused
buffer), each for the soft stream (likelihood vectors 0.05 + U[0, 1)) and for
the hard stream on the arg-max codes of the same vectors:
  soft_push1024_L0 / _L16, hard_push1024_L0 / _L16   one push of 1024 steps
  soft_push16_L0   / _L16, hard_push16_L0   / _L16   64 pushes of 16 steps
  soft_push1_L0    / _L16, hard_push1_L0    / _L16   1024 pushes of one step
and the batched soft entry points on the same vectors in the same session:
  filter_soft   nipamd_filter_soft, the comparator of L = 0
  fb_soft       nipamd_fb_soft -- one backward pass, not sixteen per row:
                context for L = 16, not a target

The protocol is profiles/stream/measure.py's: one process; every variant is
warmed up until a second of passes has run; a timed window is --batch
back-to-back passes between two device events; --reps windows per variant, the
variants alternating; median, min and max.  Writes one JSON document (--out,
default next to this script) and prints it.  Needs the GPU: there is no
fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

T_TOTAL = 1024


def warm(fn, torch):
    t0 = time.time()
    n = 0
    while n < 3 or time.time() - t0 < 1.0:               # code objects, tables, clocks
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


def timed(fns, reps, batch, torch):
    """fns: {name: callable}; windows alternate between the variants."""
    warmups = {}
    for k, f in fns.items():
        warmups[k] = warm(f, torch)
        print("warmed up %s (%d passes)" % (k, warmups[k]), file=sys.stderr, flush=True)
    ms = {k: [] for k in fns}
    for i in range(reps):
        for k, f in fns.items():
            ms[k].append(window(f, batch, torch))
        print("window %d / %d" % (i + 1, reps), file=sys.stderr, flush=True)
    out = {}
    for k, v in ms.items():
        v = np.asarray(v)
        out[k] = {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()),
                  "reps": reps, "passes_per_window": batch, "warmup_passes": warmups[k]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--B", default="4096,131072")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "measure.json"))
    args = ap.parse_args()
    import torch
    import nip_amd
    from nip_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing measured")
    N = M = 16
    nodes, pots = synth.hmm_spec(N, M)
    m = nip_amd.Model.from_spec(nodes, pots)
    P1, M1 = m.variable("P1"), m.variable("M1")
    doc = {"device": torch.cuda.get_device_name(0), "N": N, "M": M, "steps_per_pass": T_TOTAL,
           "stream_chunk": nip_amd.STREAM_CHUNK, "shapes": {}}
    for B in [int(x) for x in args.B.split(",")]:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        lik = torch.rand((B, T_TOTAL, M), dtype=torch.float64, device="cuda", generator=gen) + 0.05
        obs = lik.argmax(dim=2).to(torch.int32).unsqueeze(-1).contiguous()
        post = torch.empty((B, T_TOTAL, N), dtype=torch.float64, device="cuda")
        ll = torch.empty(B, dtype=torch.float64, device="cuda")
        st = torch.empty(B, dtype=torch.int32, device="cuda")
        cut = lambda x, T: [x[:, a:a + T].contiguous() for a in range(0, T_TOTAL, T)]
        lpieces = {T_TOTAL: [lik], 16: cut(lik, 16), 1: cut(lik, 1)}
        opieces = {T_TOTAL: [obs], 16: cut(obs, 16), 1: cut(obs, 1)}
        streams, fns, kernels = {}, {}, {}

        def stream_pass(soft, L, T):
            key = ("soft" if soft else "hard", L)
            if key not in streams:
                streams[key] = nip_amd.Stream(m, [], [P1], B, lag=L, soft_vars=[M1]) if soft else \
                    nip_amd.Stream(m, [M1], [P1], B, lag=L)
            s, flat, name = streams[key], post.view(-1), "%s_push%d_L%d" % (key[0], T, L)

            def run():
                s.reset()
                for i in range(T_TOTAL // T):
                    E = max(0, s.pending + T - L)
                    out = flat[:B * E * N].view(B, E, N)
                    if soft:
                        s.push(None, post=out, lik=lpieces[T][i])
                    else:
                        s.push(opieces[T][i], post=out)
                kernels[name] = nip_amd.last_kernel()
            return name, run

        for soft in (True, False):
            for L in (0, 16):
                for T in (T_TOTAL, 16, 1):
                    name, run = stream_pass(soft, L, T)
                    fns[name] = run

        def run_filter():
            nip_amd.forward_inference_soft(m, None, [], lik, [M1], [P1], post=post, ll=ll, status=st)
            kernels["filter_soft"] = nip_amd.last_kernel()

        def run_fb():
            nip_amd.forward_backward_inference_soft(m, None, [], lik, [M1], [P1], post=post, ll=ll, status=st)
            kernels["fb_soft"] = nip_amd.last_kernel()

        fns["filter_soft"], fns["fb_soft"] = run_filter, run_fb
        r = {"B": B}
        r.update(timed(fns, args.reps, args.batch, torch))
        for k in fns:
            pushes = T_TOTAL // int(k[k.index("push") + 4:k.rindex("_")]) if "push" in k else 1
            r[k]["kernel"] = kernels[k]
            r[k]["launches_per_pass"] = pushes
            r[k]["us_per_push"] = r[k]["median_ms"] * 1e3 / pushes
            r[k]["seq_ts_per_s"] = B * T_TOTAL / (r[k]["median_ms"] * 1e-3)
        for L in (0, 16):
            for T in (T_TOTAL, 16, 1):
                r["soft_over_hard_push%d_L%d" % (T, L)] = \
                    r["soft_push%d_L%d" % (T, L)]["median_ms"] / r["hard_push%d_L%d" % (T, L)]["median_ms"]
        r["L0_over_filter_soft"] = r["soft_push1024_L0"]["median_ms"] / r["filter_soft"]["median_ms"]
        r["L16_over_fb_soft"] = r["soft_push1024_L16"]["median_ms"] / r["fb_soft"]["median_ms"]
        # per row: L + 2 mat-vecs and one evidence evaluation at lag L, one of each at L = 0
        for T in (T_TOTAL, 16, 1):
            r["soft_L16_over_L0_push%d" % T] = \
                r["soft_push%d_L16" % T]["median_ms"] / r["soft_push%d_L0" % T]["median_ms"]
        doc["shapes"]["B%d" % B] = r
        for s in streams.values():
            s.close()
        del lik, obs, post, lpieces, opieces
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
