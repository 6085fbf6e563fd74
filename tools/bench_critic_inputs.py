#!/usr/bin/env python3
"""Time the MI355X critic-input assembly (critic_inputs.critic_inputs over csrc/mm_critic.hip) against the reference's block
(trainer.py:370-411 and :429-431) restated in eager fp32 torch on the GPU -- its three compositions, detached copies, two cats and
the two gradient-penalty interpolates with alphas drawn by numpy on the host and uploaded -- per call, with HIP events: warm-up
first, then the median of repeated runs, ours and eager alternating.  Not called by bench.py.

    python tools/bench_critic_inputs.py --out profiles/critic_inputs_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_critic_inputs.py --only ours --reps 5       # kernel times

Two timings per shape and unmask mode: "fwd" (the block under no_grad) and "fwd_bwd" (the block, then backward of sum(w * g_batch)
with fixed random w into the two fakes, which are NHWC-dense leaves like a render's image).  Algorithmic bytes per image of H*W
pixels and C output channels: the forward reads 3 * 16 and writes 3 * 4C (the D batch, which contains the G batch) + 2 * 4C (the
interpolates); the backward reads the gradient of the G batch (2 * 4C) and, for unmask 0, the two fakes (2 * 16), and writes two
gradients (2 * 16).  "copy_frac" = bytes / time over the measured 6.29 TB/s copy rate."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
SHAPES = [("config2", 48, 128, 128), ("config3", 48, 256, 256), ("config2x8", 384, 128, 128), ("market", 48, 128, 64)]


def channel_map(X, unmask):
    if unmask == 0:
        rgb, m = X[:, :3], X[:, 3:4]
        return rgb * m + torch.ones_like(rgb) * (1 - m)
    return X[:, :3] if unmask == 1 else X


def eager_block(Xa, Xer90, Xir, unmask):
    """the D batch, the two interpolates and the G batch as eager torch builds them, alphas drawn on the host"""
    B, dev = Xa.shape[0], Xa.device
    Ma, M1, M2 = channel_map(Xa, unmask), channel_map(Xer90, unmask), channel_map(Xir, unmask)
    real, f1, f2 = Ma.detach().clone(), M1.detach().clone(), M2.detach().clone()
    d_batch = torch.cat((real, f1, f2), 0)
    gps = []
    for fake in (f1, f2):
        a = torch.tensor(np.random.random((B, 1, 1, 1)), dtype=torch.float32, device=dev)
        gps.append((a * real + ((1 - a) * fake)).requires_grad_(True))
    g_batch = torch.cat((M1, M2), 0)
    return d_batch, g_batch, gps[0], gps[1]


def timed(fn, ev):
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--only", choices=["both", "ours"], default="both")
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into SHAPES")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    pkg = importlib.import_module("3d-magic-mirror_amd")
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for si in [int(s) for s in a.shapes.split(",")]:
        name, B, H, W = SHAPES[si]
        g = torch.Generator(device=dev).manual_seed(si)
        nhwc = lambda: torch.rand(B, H, W, 4, generator=g, device=dev).permute(0, 3, 1, 2)  # noqa: E731
        Xa = nhwc().contiguous()                                      # the data loader's batch is NCHW
        leaves = [nhwc().requires_grad_(), nhwc().requires_grad_()]   # the renders' images are NHWC memory
        for unmask in (0, 2):
            C = 4 if unmask == 2 else 3
            w = torch.randn(2 * B, C, H, W, generator=g, device=dev)

            def ours():
                ci = pkg.critic_inputs(Xa, leaves[0], leaves[1], unmask=unmask)
                return ci.g_batch

            def theirs():
                return eager_block(Xa, leaves[0], leaves[1], unmask)[1]

            impls = [("ours", ours)] + ([("eager", theirs)] if a.only == "both" else [])

            def fwd(f):
                with torch.no_grad():
                    f()

            def fwdbwd(f):
                (f() * w).sum().backward()

            res = {}
            for mode, run in (("fwd", fwd), ("fwd_bwd", fwdbwd)):
                for _ in range(a.warmup):
                    for _, f in impls:
                        run(f)
                torch.cuda.synchronize()
                times = {k: [] for k, _ in impls}
                for rep in range(a.reps):                            # alternating: drift hits both alike
                    for k, f in impls:
                        for t in leaves:
                            t.grad = None
                        np.random.seed(rep)
                        times[k].append(timed(lambda: run(f), ev))
                for k in times:
                    res["%s_%s_us" % (k, mode)] = float(np.median(times[k]))
            fwd_bytes = B * H * W * (48 + 20 * C)
            bwd_bytes = B * H * W * (8 * C + 32 + (32 if unmask == 0 else 0))
            row = {"shape": name, "B": B, "H": H, "W": W, "unmask": unmask, "fwd_bytes": fwd_bytes, "fwd_bwd_bytes": fwd_bytes + bwd_bytes, **res}
            for mode, nbytes in (("fwd", fwd_bytes), ("fwd_bwd", fwd_bytes + bwd_bytes)):
                row["ours_%s_copy_frac" % mode] = nbytes / (res["ours_%s_us" % mode] * 1e-6) / COPY_RATE
                if "eager_%s_us" % mode in res:
                    row["speedup_%s" % mode] = res["eager_%s_us" % mode] / res["ours_%s_us" % mode]
            rows.append(row)
            print(json.dumps(row), flush=True)
        del leaves, Xa, w
        torch.cuda.empty_cache()
    out = {"tool": "tools/bench_critic_inputs.py", "warmup": a.warmup, "reps": a.reps, "copy_rate_Bps": COPY_RATE,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"critic_inputs": [(r["shape"], r["unmask"], round(r.get("speedup_fwd", 0), 2), round(r.get("speedup_fwd_bwd", 0), 2))
                                        for r in rows]}))


if __name__ == "__main__":
    main()
