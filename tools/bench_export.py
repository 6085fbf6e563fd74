#!/usr/bin/env python3
"""Time the MI355X export of renders to 8-bit pixels (export.export_grid / export_images over csrc/mm_export.hip) against the eager
composition the reference performs, restated in fp32 torch on the same GPU, per call, with HIP events: warm-up first, then the median
of repeated runs, ours and eager alternating.  Not called by bench.py.

    python tools/bench_export.py --out profiles/export_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_export.py --only ours --reps 5 --wall-reps 0      # kernel times

Two cases per shape:
  "grid"    the 36 contact sheets of a turntable (trainer.py:616-631) from a (B,36,4,H,W) NHWC tensor, what render_views returns.
            Eager: per frame make_grid (restated: new_full + one copy per image) of x[:, n, :3], permute to HWC, * 255, .to(uint8).
  "images"  rgb + mask of a (B,4,H,W) NHWC render (trainer.py:727-766).  Eager: per image X[i, :3].mul(255).byte() and
            X[i, 3].mul(255).byte().
Algorithmic bytes: every input pixel read once (16 bytes) and every output byte written once.  "copy_frac" = bytes / time over the
measured 6.29 TB/s copy rate.  "wall" times (perf_counter around a synchronised call, median of --wall-reps) include bringing the
result to the host: ours is the launch and ONE .cpu() of bytes; the reference's is what its loop does -- per frame (per image) a float
.cpu() and the multiply and cast on the host."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
VIEWS = 36
SHAPES = [("config2", 48, 128, 128), ("config3", 48, 256, 256), ("config2x8", 384, 128, 128), ("market", 48, 128, 64)]


def make_grid(x, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid for a (B,3,H,W) batch, restated [recall-risk: from memory, torchvision is not installed]"""
    B, C, H, W = x.shape
    if B == 1:
        return x[0]
    xmaps = min(nrow, B)
    ymaps = -(-B // xmaps)
    grid = x.new_full((C, (H + padding) * ymaps + padding, (W + padding) * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for xx in range(xmaps):
            if k >= B:
                break
            grid.narrow(1, y * (H + padding) + padding, H).narrow(2, xx * (W + padding) + padding, W).copy_(x[k])
            k += 1
    return grid


def eager_grid(x):
    return [(make_grid(x[:, n, :3]).permute(1, 2, 0) * 255).to(torch.uint8) for n in range(x.shape[1])]


def eager_images(x):
    return [(x[i, :3].mul(255).byte(), x[i, 3].mul(255).byte()) for i in range(x.shape[0])]


def reference_grid_to_host(x):
    out = []
    for n in range(x.shape[1]):
        image = make_grid(x[:, n, :3]).permute(1, 2, 0).cpu().numpy()
        out.append((image * 255.0).astype(np.uint8))
    return out


def reference_images_to_host(x):
    return [(x[i, :3].detach().cpu().mul(255).byte(), x[i, 3].detach().cpu().mul(255).byte()) for i in range(x.shape[0])]


def timed(fn, ev):
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3          # us


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--wall-reps", type=int, default=3)
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
        Hg, Wg = pkg.grid_shape(B, H, W)
        cases = (("grid", (B, VIEWS, H, W, 4), lambda x: pkg.export_grid(x), eager_grid, reference_grid_to_host,
                  B * VIEWS * H * W * 16 + VIEWS * Hg * Wg * 3),
                 ("images", (B, H, W, 4), lambda x: pkg.export_images(x, "rgb+mask"), eager_images, reference_images_to_host,
                  B * H * W * (16 + 4)))
        for case, shape, ours, eager, reference, nbytes in cases:
            x = torch.rand(shape, generator=g, device=dev).movedim(-1, -3)       # NHWC memory, like a render
            impls = [("ours", lambda: ours(x))] + ([("eager", lambda: eager(x))] if a.only == "both" else [])
            for _ in range(a.warmup):
                for _, f in impls:
                    f()
            torch.cuda.synchronize()
            times = {k: [] for k, _ in impls}
            for _ in range(a.reps):                                    # alternating: drift hits both alike
                for k, f in impls:
                    times[k].append(timed(f, ev))
            row = {"shape": name, "case": case, "B": B, "H": H, "W": W, "views": VIEWS if case == "grid" else 1, "bytes": nbytes}
            for k in times:
                row["%s_us" % k] = float(np.median(times[k]))
            row["ours_copy_frac"] = nbytes / (row["ours_us"] * 1e-6) / COPY_RATE
            if "eager_us" in row:
                row["speedup"] = row["eager_us"] / row["ours_us"]
            if a.wall_reps:
                to_host = lambda: [t.cpu() for t in (lambda r: r if isinstance(r, tuple) else (r,))(ours(x))]  # noqa: E731
                walls = [("ours", to_host)] + ([("reference", lambda: reference(x))] if a.only == "both" else [])
                wt = {k: [] for k, _ in walls}
                for _ in range(a.wall_reps):
                    for k, f in walls:
                        wt[k].append(wall(f))
                for k in wt:
                    row["%s_to_host_wall_us" % k] = float(np.median(wt[k]))
                if "reference_to_host_wall_us" in row:
                    row["speedup_to_host_wall"] = row["reference_to_host_wall_us"] / row["ours_to_host_wall_us"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            del x
            torch.cuda.empty_cache()
    out = {"tool": "tools/bench_export.py", "warmup": a.warmup, "reps": a.reps, "wall_reps": a.wall_reps, "copy_rate_Bps": COPY_RATE,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"export": [(r["shape"], r["case"], round(r.get("speedup", 0), 2), round(r.get("speedup_to_host_wall", 0), 2)) for r in rows]}))


if __name__ == "__main__":
    main()
