#!/usr/bin/env python3
"""Time the MI355X JPEG round trip (jpeg.jpeg_roundtrip over csrc/mm_jpeg.hip) against what a user has without it, by the wall clock until
the decoded frames are usable on the device: warm-up first, then --runs alternating runs of --reps calls each, the median and the range of
each form.  Not called by bench.py.

    python tools/bench_jpeg_roundtrip.py --out profiles/jpeg_roundtrip_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_jpeg_roundtrip.py --only ours --shape market --runs 2      # kernel times, a run per shape

B = 48 frames made by pyramid_frames with the tool/generate_market_test preset (tools/bench_jpeg.py's frames), at Market's 128 x 64 and at
128 x 128, quality 100.  Three forms, all from frames in device memory to decoded uint8 frames (B,H,W,3) in device memory, synchronised:
  "ours"     jpeg_roundtrip(frames): three launches (transform, idct, pixels), no copy.
  "pillow"   the yardstick of today: encode_jpeg(frames) (the files in host memory), then per file
             Image.open(BytesIO(file)).convert('RGB') on the host, one process, then ONE upload of the stacked frames.
  "pool"     the same with the files decoded by a pool of 16 processes (started before the clock, and before this process touches the GPU):
             the files go to the workers in 16 pieces and the frames come back.
"ours_L" is also timed (the masks' round trip, mode "L", of the frames' first channel: one launch); it has no yardstick row of its own.
The forms give the same frames, byte for byte; that is asserted before anything is timed.  "bar" says whether ours' slowest run is under
the single-process yardstick's fastest, "bar_pool" the same against the pool.  --kernel-us records kernel times measured separately (the
rocprofv3 line above: the sum over the three kernels of one call) and their share of the call."""
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
SITE = "tool/generate_market_test"
WORKERS = 16


def pillow_decode(files):
    """(n,H,W,3) uint8 on the host from a list of files: the evaluation's loop"""
    from PIL import Image
    out = []
    for data in files:
        with Image.open(io.BytesIO(data)) as im:
            out.append(np.asarray(im.convert("RGB")))
    return np.stack(out)


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
    ap.add_argument("--shape", choices=[s[0] for s in SHAPES], default=None, help="one shape only (a profiler run per shape)")
    ap.add_argument("--kernel-us", default="", help="shape=us,... device time of one call from a separate rocprofv3 run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pool = multiprocessing.get_context("spawn").Pool(WORKERS) if a.only == "all" else None      # before the GPU is opened; the workers never open it
    import torch
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    pkg = importlib.import_module("3d-magic-mirror_amd")
    P = importlib.import_module("3d-magic-mirror_amd.pyramid")
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
        masks = frames[..., 0].contiguous()
        torch.cuda.synchronize()

        def ours():
            out = pkg.jpeg_roundtrip(frames)
            torch.cuda.synchronize()
            return out

        def ours_L():
            out = pkg.jpeg_roundtrip(masks, mode="L")
            torch.cuda.synchronize()
            return out

        def pillow():
            out = torch.from_numpy(pillow_decode(list(pkg.encode_jpeg(frames)))).to(dev)
            torch.cuda.synchronize()
            return out

        def pooled():
            files = list(pkg.encode_jpeg(frames))
            step = (len(files) + WORKERS - 1) // WORKERS
            parts = pool.map(pillow_decode, [files[i:i + step] for i in range(0, len(files), step)])
            out = torch.from_numpy(np.concatenate(parts)).to(dev)
            torch.cuda.synchronize()
            return out

        impls = [("ours", ours), ("ours_L", ours_L)]
        if a.only == "all":
            impls += [("pillow", pillow), ("pool", pooled)]
            want = ours()
            assert torch.equal(want, pillow()) and torch.equal(want, pooled()), "the three forms must give the same frames"
        for _ in range(a.warmup):
            for _, f in impls:
                f()
        times = {k: [] for k, _ in impls}
        for _ in range(a.runs):                                                               # alternating: drift hits all alike
            for k, f in impls:
                times[k].append(float(np.mean([wall(f) for _ in range(a.reps)])))
        row = {"shape": name, "site": SITE, "B": B, "H": H, "W": W, "quality": 100,
               "mean_abs_change_grey_levels": float((ours().float() - frames.float()).abs().mean())}
        for k in times:
            row["%s_us" % k] = float(np.median(times[k]))
            row["%s_min_us" % k], row["%s_max_us" % k] = float(np.min(times[k])), float(np.max(times[k]))
            row["%s_runs_us" % k] = times[k]
        if "pillow_us" in row:
            row["frames_equal_pillow"] = True
            row["speedup_vs_pillow"] = row["pillow_us"] / row["ours_us"]
            row["speedup_vs_pool"] = row["pool_us"] / row["ours_us"]
            row["bar"] = bool(row["ours_max_us"] < row["pillow_min_us"])
            row["bar_pool"] = bool(row["ours_max_us"] < row["pool_min_us"])
        if name in kernel_us:
            row["device_us"] = kernel_us[name]
            row["device_share_of_call"] = kernel_us[name] / row["ours_us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if pool is not None:
        pool.close()
        pool.join()
    out = {"tool": "tools/bench_jpeg_roundtrip.py", "warmup": a.warmup, "runs": a.runs, "reps": a.reps, "workers": WORKERS,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"jpeg_roundtrip": [(r["shape"], round(r.get("speedup_vs_pillow", 0), 2), r.get("bar"), round(r.get("speedup_vs_pool", 0), 2),
                                          r.get("bar_pool")) for r in rows]}))


if __name__ == "__main__":
    main()
