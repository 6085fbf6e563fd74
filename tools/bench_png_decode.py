#!/usr/bin/env python3
"""Time the MI355X PNG decoder (png_decode.decode_png over csrc/mm_png_decode.hip) against Pillow, by the wall clock from the files' bytes
in host memory to the frames usable in device memory: warm-up first, then --runs alternating runs of --reps calls, the median and the range
of each form.  Not called by bench.py.

    python tools/bench_png_decode.py --out profiles/png_decode_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_png_decode.py --only ours --workload cub --runs 1 --reps 2      # kernel times

Workloads (1024 files -- 128 distinct ones, eight times over -- written by Pillow at its default compression level from seeded blob-like
content):
  "cub"      L masks of 500 x 375 (CUB's shape)
  "market"   L masks of 128 x 64 (Market-1501's shape)
  "rgba"     RGBA files of 128 x 128
Forms:
  "ours"         decode_png(files, mode): walk the chunks on the host, one upload, one memset, three launches; the clock stops when the
                 status words are back (strict=True), so every kernel has finished.  "ours_lower" times the host walk (lower_png_decode)
                 alone: it is part of "ours".
  "pillow"       what a user has without it: per file np.asarray(Image.open(BytesIO(b)).convert(mode)) in one process, the arrays
                 concatenated, one upload
  "pillow_pool"  the same decode in a pool of 16 processes (started before the GPU is touched and never touching it), one upload
Before anything is timed every frame of ours must equal Pillow's.  No pass mark is fixed: the ratios are reported as they come out."""
import argparse
import functools
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

POOL = 16
WORKLOADS = {"cub": ("L", 375, 500), "market": ("L", 128, 64), "rgba": ("RGBA", 128, 128)}      # mode, H, W


def pillow_decode(mode, data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert(mode))


def blobs(rng, h, w):
    """a mask-like image: a few soft blobs, thresholded into a handful of grey levels"""
    y, x = np.mgrid[:h, :w]
    a = np.zeros((h, w))
    for _ in range(5):
        cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.08, 0.3) * max(h, w)
        a += np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
    return (np.clip(a / a.max() * 1.6, 0, 1) * 255).astype(np.uint8)


def workload(name, n=1024, distinct=128):
    from PIL import Image
    mode, h, w = WORKLOADS[name]
    rng = np.random.default_rng(sorted(WORKLOADS).index(name) + 1)
    files = []
    for _ in range(distinct):
        g = blobs(rng, h, w)
        if mode == "RGBA":
            g = np.stack([g, 255 - g, blobs(rng, h, w), ((g > 40) * 255).astype(np.uint8)], 2)
        else:
            g = ((g > 90) * 255).astype(np.uint8) if rng.random() < 0.5 else g          # half hard masks, half soft ones
        f = io.BytesIO()
        Image.fromarray(g).save(f, "PNG")
        files.append(f.getvalue())
    return mode, files * (n // distinct)


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e6          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of every form")
    ap.add_argument("--reps", type=int, default=20, help="calls of ours per run; a run's time is their mean")
    ap.add_argument("--only", choices=["all", "ours"], default="all")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default=None, help="one workload only (a profiler run per workload)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pool = multiprocessing.get_context("spawn").Pool(POOL) if a.only == "all" else None      # before the GPU is initialised; the workers never import torch
    try:
        import torch
        assert torch.cuda.is_available(), "the benchmark needs the GPU"
        pkg = importlib.import_module("3d-magic-mirror_amd")
        dev = torch.device("cuda:0")

        def upload(arrays):
            out = torch.from_numpy(np.concatenate([x.reshape(-1) for x in arrays])).to(dev)
            torch.cuda.synchronize()
            return out

        rows = []
        for name in ("cub", "market", "rgba"):
            if a.workload not in (None, name):
                continue
            mode, files = workload(name)
            low = pkg.lower_png_decode(files, mode)
            one = functools.partial(pillow_decode, mode)
            impls = [("ours", lambda: pkg.decode_png(files, mode, device=dev)), ("ours_lower", lambda: pkg.lower_png_decode(files, mode))]
            if a.only == "all":
                want = upload([one(f) for f in files])
                assert torch.equal(pkg.decode_png(files, mode, device=dev).images, want), "every frame of %s must equal Pillow's" % name
                impls.append(("pillow", lambda: upload([one(f) for f in files])))
                impls.append(("pillow_pool", lambda: upload(pool.map(one, files, chunksize=max(1, len(files) // (4 * POOL))))))
                assert torch.equal(impls[-1][1](), want)
            for _ in range(a.warmup):
                for k, f in impls:
                    f()
            times = {k: [] for k, _ in impls}
            for _ in range(a.runs):                                                           # alternating: drift hits all alike
                for k, f in impls:
                    times[k].append(float(np.mean([wall(f) for _ in range(a.reps if k.startswith("ours") else 1)])))
            row = {"workload": name, "mode": mode, "n": len(files), "file_bytes_total": int(sum(len(f) for f in files)),
                   "deflate_bytes_total": int(low["data"].size), "stream_bytes_total": int(low["stream_bytes"]), "pixels_total": int(low["offsets"][-1])}
            for k in times:
                row["%s_us" % k] = float(np.median(times[k]))
                row["%s_min_us" % k], row["%s_max_us" % k] = float(np.min(times[k])), float(np.max(times[k]))
                row["%s_runs_us" % k] = times[k]
            if "pillow_us" in row:
                row["speedup_vs_pillow"] = row["pillow_us"] / row["ours_us"]
                row["speedup_vs_pillow_pool"] = row["pillow_pool_us"] / row["ours_us"]
                row["ours_slowest_under_pillow_fastest"] = row["ours_max_us"] < row["pillow_min_us"]
                row["ours_slowest_under_pillow_pool_fastest"] = row["ours_max_us"] < row["pillow_pool_min_us"]
            rows.append(row)
            print(json.dumps(row), flush=True)
        out = {"tool": "tools/bench_png_decode.py", "warmup": a.warmup, "runs": a.runs, "reps": a.reps, "pool": POOL,
               "device": torch.cuda.get_device_name(0), "rows": rows}
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        print(json.dumps({"png_decode": [(r["workload"], round(r.get("speedup_vs_pillow", 0), 2), round(r.get("speedup_vs_pillow_pool", 0), 2)) for r in rows]}))
    finally:
        if pool is not None:
            pool.close()
            pool.join()


if __name__ == "__main__":
    main()
