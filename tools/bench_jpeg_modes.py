#!/usr/bin/env python3
"""Time the MI355X JPEG encoder's layouts beyond 4:2:0 (jpeg.encode_jpeg with mode / subsampling over csrc/mm_jpeg.hip) against Pillow,
by the wall clock until the files are in host memory: warm-up first, then --runs alternating runs of --reps calls each, the median and the
range of each form.  tools/bench_jpeg.py is the same for the default layout.  Not called by bench.py.

    python tools/bench_jpeg_modes.py --out profiles/jpeg_modes_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_jpeg_modes.py --only ours --shape market --layout L --runs 2     # kernel times

B = 48 at Market's 128 x 64 and at 128 x 128, quality 100.  Layout "L": the masks the evaluation loop writes, export_images(gt, "mask") of
synthetic ground truth (a silhouette with a soft edge).  Layouts "4:4:4" and "4:2:2": the frames of tools/bench_jpeg.py, pyramid_frames
with the tool/generate_market_test preset.  Three forms per layout and shape:
  "ours"     encode_jpeg(x, mode=..., subsampling=...) on bytes in device memory: one memset and eight launches, then two device-to-host
             copies (offsets, bytes).  The clock stops when the JpegBatch is returned: the files are in host memory.
  "pillow"   per image Image.fromarray(f).save(BytesIO, 'JPEG', quality=100[, subsampling=s]) from arrays ALREADY on the host, one
             process.  (The scripts' device-to-host copy before it is left out: it favours this side.)
  "pool"     the same over a pool of 16 processes (started before the clock, and before this process touches the GPU): the arrays go to
             the workers in 16 pieces and the files come back.
The forms make the same files, byte for byte; that is asserted before anything is timed.  "bar" says whether ours' slowest run is under
the single-process yardstick's fastest, "bar_pool" the same against the pool.  --kernel-us records kernel times measured separately (the
rocprofv3 line above: the sum over the eight kernels and the memset of one call) and their share of the call."""
import argparse
import importlib
import io
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("market", 48, 128, 64), ("config2", 48, 128, 128)]
LAYOUTS = ["L", "4:4:4", "4:2:2"]
SITE = "tool/generate_market_test"
WORKERS = 16


def pillow_files(job):
    """a list of files from (layout, (n,H,W) or (n,H,W,3) uint8 on the host): the scripts' loop"""
    from PIL import Image
    layout, frames = job
    kw = {} if layout == "L" else {"subsampling": layout}
    out = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=100, **kw)
        out.append(buf.getvalue())
    return out


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e6          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of every form")
    ap.add_argument("--reps", type=int, default=20, help="calls per run; a run's time is their mean")
    ap.add_argument("--only", choices=["all", "ours"], default="all")
    ap.add_argument("--shape", choices=[s[0] for s in SHAPES], default=None, help="one shape only (a profiler run per shape and layout)")
    ap.add_argument("--layout", choices=LAYOUTS, default=None, help="one layout only")
    ap.add_argument("--kernel-us", default="", help="layout/shape=us,... device time of one call from a separate rocprofv3 run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pool = multiprocessing.get_context("spawn").Pool(WORKERS) if a.only == "all" else None      # before the GPU is opened; the workers never open it
    import torch
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    pkg = importlib.import_module("3d-magic-mirror_amd")
    P = importlib.import_module("3d-magic-mirror_amd.pyramid")
    S = importlib.import_module("3d-magic-mirror_amd.synthetic")
    dev = torch.device("cuda:0")
    kernel_us = {k: float(v) for k, v in (kv.split("=") for kv in a.kernel_us.split(",") if kv)}
    rows = []
    for si, (name, B, H, W) in enumerate(SHAPES):
        if a.shape not in (None, name):
            continue
        g = torch.Generator(device=dev).manual_seed(si)
        pred = torch.rand((B, H, W, 4), generator=g, device=dev).movedim(-1, -3)
        pred[:, 3] = (pred[:, 3] * 2 - 0.5).clamp(0, 1)
        Xa = torch.rand((B, 4, H, W), generator=g, device=dev)
        hg = torch.Generator().manual_seed(si)
        frames = pkg.pyramid_frames(pred, Xa, torch.randint(0, B, (B,), generator=hg), **P.preset(SITE, B, generator=hg))
        gt = S.synthetic_batch(torch.zeros(4, 3), B, H, W, seed=si)[1].float().contiguous().to(dev)
        masks = pkg.export_images(gt, "mask", rounding="trunc")
        for layout in LAYOUTS:
            if a.layout not in (None, layout):
                continue
            x = masks if layout == "L" else frames
            kw = dict(mode="L") if layout == "L" else dict(subsampling=layout)
            host = x.cpu().numpy()
            pieces = [(layout, p) for p in np.array_split(host, WORKERS) if len(p)]
            torch.cuda.synchronize()
            impls = [("ours", lambda: pkg.encode_jpeg(x, **kw))]
            if a.only == "all":
                impls += [("pillow", lambda: pillow_files((layout, host))), ("pool", lambda: [f for part in pool.map(pillow_files, pieces) for f in part])]
                files = list(impls[0][1]())
                assert files == impls[1][1]() == impls[2][1](), "the three forms must make the same files"
            for _ in range(a.warmup):
                for _, f in impls:
                    f()
            times = {k: [] for k, _ in impls}
            for _ in range(a.runs):                                                           # alternating: drift hits all alike
                for k, f in impls:
                    times[k].append(float(np.mean([wall(f) for _ in range(a.reps)])))
            batch = impls[0][1]()
            row = {"layout": layout, "shape": name, "input": "export_images(gt, 'mask')" if layout == "L" else SITE, "B": B, "H": H, "W": W,
                   "quality": 100, "file_bytes_total": int(batch.offsets[-1])}
            for k in times:
                row["%s_us" % k] = float(np.median(times[k]))
                row["%s_min_us" % k], row["%s_max_us" % k] = float(np.min(times[k])), float(np.max(times[k]))
                row["%s_runs_us" % k] = times[k]
            if "pillow_us" in row:
                row["files_equal_pillow"] = True
                row["speedup_vs_pillow"] = row["pillow_us"] / row["ours_us"]
                row["speedup_vs_pool"] = row["pool_us"] / row["ours_us"]
                row["bar"] = bool(row["ours_max_us"] < row["pillow_min_us"])
                row["bar_pool"] = bool(row["ours_max_us"] < row["pool_min_us"])
            key = "%s/%s" % (layout, name)
            if key in kernel_us:
                row["device_us"] = kernel_us[key]
                row["device_share_of_call"] = kernel_us[key] / row["ours_us"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if pool is not None:
        pool.close()
        pool.join()
    out = {"tool": "tools/bench_jpeg_modes.py", "warmup": a.warmup, "runs": a.runs, "reps": a.reps, "workers": WORKERS,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"jpeg_modes": [(r["layout"], r["shape"], round(r.get("speedup_vs_pillow", 0), 2), r.get("bar"), round(r.get("speedup_vs_pool", 0), 2),
                                      r.get("bar_pool")) for r in rows]}))


if __name__ == "__main__":
    main()
