#!/usr/bin/env python3
"""Time the MI355X JPEG decoder (jpeg_decode.decode_jpeg over csrc/mm_jpeg_decode.hip) against Pillow, by the wall clock from the files'
bytes in host memory to the frames in device memory: warm-up first, then --runs alternating runs, the median and the range of each form.
Not called by bench.py.

    python tools/bench_jpeg_decode.py --out profiles/jpeg_decode_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_jpeg_decode.py --only ours --workload market --runs 2      # kernel times

Workloads (files written by Pillow from seeded render-like images: smooth colour fields with a little noise):
  "market"   4096 files of 128 x 64 at quality 95 (Market-1501's shape)
  "atr"      512 files of mixed sizes, 100..400 pixels a side, quality 90 (ATR-like)
  "atr_rst"  the same images saved with restart_marker_rows=1: an interval per MCU row, so many more segments in flight
Forms:
  "ours"         decode_jpeg(files): parse on the host, one upload, one memset, three launches; the clock stops when the status words are
                 back (strict=True), so every kernel has finished.  "ours_lower" times the host parse (lower_jpeg_decode) alone: it is
                 part of "ours".
  "pillow"       what a user has without it: per file np.asarray(Image.open(BytesIO(b)).convert('RGB')) in one process, the arrays
                 concatenated, one upload
  "pillow_pool"  the same decode in a pool of 16 processes (started before the GPU is touched and never touching it), one upload
Before anything is timed every frame of ours must equal Pillow's.  No pass mark is fixed: the ratios are reported as they come out."""
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

POOL = 16


def pillow_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def image(rng, h, w):
    """a render-like image: a coarse random colour field, enlarged, with a little noise"""
    coarse = rng.integers(0, 256, (h // 16 + 2, w // 16 + 2, 3)).astype(np.float32)
    y, x = np.linspace(0, coarse.shape[0] - 1.001, h), np.linspace(0, coarse.shape[1] - 1.001, w)
    y0, x0 = y.astype(int), x.astype(int)
    fy, fx = (y - y0)[:, None, None], (x - x0)[None, :, None]
    a = coarse[y0][:, x0] * (1 - fx) + coarse[y0][:, x0 + 1] * fx
    b = coarse[y0 + 1][:, x0] * (1 - fx) + coarse[y0 + 1][:, x0 + 1] * fx
    return np.clip(a * (1 - fy) + b * fy + rng.normal(0, 4, (h, w, 3)), 0, 255).astype(np.uint8)


def workload(name):
    from PIL import Image
    rng = np.random.default_rng({"market": 1, "atr": 2, "atr_rst": 2}[name])
    files = []
    for _ in range(4096 if name == "market" else 512):
        h, w = (128, 64) if name == "market" else (int(v) for v in rng.integers(100, 401, 2))
        f = io.BytesIO()
        kw = {"quality": 95} if name == "market" else {"quality": 90}
        if name == "atr_rst":
            kw["restart_marker_rows"] = 1
        Image.fromarray(image(rng, h, w)).save(f, "JPEG", **kw)
        files.append(f.getvalue())
    return files


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e6          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of every form")
    ap.add_argument("--reps", type=int, default=3, help="calls of ours per run; a run's time is their mean")
    ap.add_argument("--only", choices=["all", "ours"], default="all")
    ap.add_argument("--workload", choices=["market", "atr", "atr_rst"], default=None, help="one workload only (a profiler run per workload)")
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
        for name in ("market", "atr", "atr_rst"):
            if a.workload not in (None, name):
                continue
            files = workload(name)
            low = pkg.lower_jpeg_decode(files)
            impls = [("ours", lambda: pkg.decode_jpeg(files, device=dev)), ("ours_lower", lambda: pkg.lower_jpeg_decode(files))]
            if a.only == "all":
                want = upload([pillow_decode(f) for f in files])
                assert torch.equal(pkg.decode_jpeg(files, device=dev).images, want), "every frame of %s must equal Pillow's" % name
                impls.append(("pillow", lambda: upload([pillow_decode(f) for f in files])))
                impls.append(("pillow_pool", lambda: upload(pool.map(pillow_decode, files, chunksize=max(1, len(files) // (4 * POOL))))))
                assert torch.equal(impls[-1][1](), want)
            for _ in range(a.warmup):
                for k, f in impls:
                    f()
            times = {k: [] for k, _ in impls}
            for _ in range(a.runs):                                                           # alternating: drift hits all alike
                for k, f in impls:
                    times[k].append(float(np.mean([wall(f) for _ in range(a.reps if k.startswith("ours") else 1)])))
            row = {"workload": name, "n": len(files), "file_bytes_total": int(sum(len(f) for f in files)), "pixels_total": int(low["offsets"][-1]),
                   "blocks": int(low["blocks"]), "segments": int((low["segments"][:, 2] > 0).sum()), "table_sets": int(len(low["sets"]))}
            for k in times:
                row["%s_us" % k] = float(np.median(times[k]))
                row["%s_min_us" % k], row["%s_max_us" % k] = float(np.min(times[k])), float(np.max(times[k]))
                row["%s_runs_us" % k] = times[k]
            if "pillow_us" in row:
                row["speedup_vs_pillow"] = row["pillow_us"] / row["ours_us"]
                row["speedup_vs_pillow_pool"] = row["pillow_pool_us"] / row["ours_us"]
            rows.append(row)
            print(json.dumps(row), flush=True)
        out = {"tool": "tools/bench_jpeg_decode.py", "warmup": a.warmup, "runs": a.runs, "reps": a.reps, "pool": POOL,
               "device": torch.cuda.get_device_name(0), "rows": rows}
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        print(json.dumps({"jpeg_decode": [(r["workload"], round(r.get("speedup_vs_pillow", 0), 2), round(r.get("speedup_vs_pillow_pool", 0), 2)) for r in rows]}))
    finally:
        if pool is not None:
            pool.close()
            pool.join()


if __name__ == "__main__":
    main()
