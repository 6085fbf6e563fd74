#!/usr/bin/env python3
"""Time the MI355X assembly of training batches (input_batches.assemble_batch over csrc/mm_batch.hip) against what else can make the
batch on the same machine, per call: warm-up first, then the median of repeated runs.  Not called by bench.py.

    python tools/bench_input_batches.py --out profiles/input_batches_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_input_batches.py --only ours --reps 5      # kernel times

  "ours"    draw_augmentation + assemble_batch for B samples of a resident pool, by HIP events ("ours_us"), and by the wall clock around
            a synchronised call ("ours_wall_us", which includes the draws and the lowering on the host).
  "eager"   the same steps composed from torch operators on the GPU, from the same resident bytes: per image flip, pad, crop, pad to
            a square, F.interpolate(mode="bicubic", antialias=True), nearest for the mask, threshold, composite; then torch.stack.
            NOT bit-equal to the loader: fp32 taps, no rounding to bytes between the passes or after them.
  "pillow"  the loader's own Pillow steps from decoded arrays, the batch spread over 16 worker processes (what a DataLoader with 16
            workers can do at best: no JPEG decoding, no collation into shared memory), by the wall clock; "not measured" if Pillow
            does not import.  The workers are started, used and closed BEFORE this process touches the GPU."""
import argparse
import importlib
import json
import multiprocessing
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("cub", "cub", 48, (375, 500), (128, 128)), ("market", "market", 48, (128, 64), (128, 64))]
POOL = 64
_DATA = {}


def make_sources(seed, hw):
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for _ in range(POOL)]
    segs = [np.where(rng.random(hw) < 0.5, 255, 0).astype(np.uint8) for _ in range(POOL)]
    return imgs, segs


def _worker_init(seed, hw):
    _DATA["imgs"], _DATA["segs"] = make_sources(seed, hw)


def _pillow_one(job):
    from PIL import Image, ImageOps
    i, recipe, aug, (H, W) = job
    im, sg = Image.fromarray(_DATA["imgs"][i], "RGB"), Image.fromarray(_DATA["segs"][i], "L")
    cut = lambda p: p > 160 and 255  # noqa: E731
    if recipe == "cub":
        flip, _, _, left, upper, right, lower = aug
        if flip:
            im, sg = im.transpose(Image.FLIP_LEFT_RIGHT), sg.transpose(Image.FLIP_LEFT_RIGHT)
        im, sg = ImageOps.expand(im, 10), ImageOps.expand(sg, 10)
        im, sg = im.crop((left, upper, right, lower)), sg.crop((left, upper, right, lower))
        w, h = im.size
        d = max(w, h)
        pad = ((d - w) // 2, (d - h) // 2, d - w - (d - w) // 2, d - h - (d - h) // 2)
        im, sg = ImageOps.expand(im, pad), ImageOps.expand(sg, pad)
    else:
        left, upper, flip = aug
        im, sg = im.resize((W, H)), sg.resize((W, H), Image.NEAREST).point(cut)
        im, sg = ImageOps.expand(im, 10), ImageOps.expand(sg, 10)
        im, sg = im.crop((left, upper, left + W, upper + H)), sg.crop((left, upper, left + W, upper + H))
        if flip:
            im, sg = im.transpose(Image.FLIP_LEFT_RIGHT), sg.transpose(Image.FLIP_LEFT_RIGHT)
    im, sg = im.resize((W, H)), sg.resize((W, H), Image.NEAREST).point(cut)
    v = np.asarray(im, dtype=np.uint8).astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)
    m = np.asarray(sg, dtype=np.uint8).astype(np.float32)[None] / np.float32(255.0)
    return np.concatenate([v * m + (1 - m), m], 0)


def eager_one(img, seg, recipe, aug, out_hw):
    import torch
    import torch.nn.functional as F
    H, W = out_hw
    x = torch.cat((img.permute(2, 0, 1), seg[None]), 0)           # (4,Hs,Ws) uint8
    if recipe == "cub":
        flip, _, _, left, upper, right, lower = aug
        if flip:
            x = x.flip(-1)
        x = F.pad(x, (10, 10, 10, 10))[:, upper:lower, left:right]
        h, w = x.shape[1:]
        d = max(w, h)
        x = F.pad(x, ((d - w) // 2, d - w - (d - w) // 2, (d - h) // 2, d - h - (d - h) // 2)).float()[None]
        v = F.interpolate(x[:, :3], size=(H, W), mode="bicubic", antialias=True, align_corners=False).clamp(0, 255) / 255
        m = (F.interpolate(x[:, 3:], size=(H, W), mode="nearest-exact") > 160).float()
    else:
        left, upper, flip = aug
        x = x.float()[None]
        v = F.interpolate(x[:, :3], size=(H, W), mode="bicubic", antialias=True, align_corners=False).clamp(0, 255) / 255
        m = (F.interpolate(x[:, 3:], size=(H, W), mode="nearest-exact") > 160).float()
        y = F.pad(torch.cat((v, m), 1), (10, 10, 10, 10))[:, :, upper:upper + H, left:left + W]
        if flip:
            y = y.flip(-1)
        v, m = y[:, :3], y[:, 3:]
    return torch.cat((v * m + (1 - m), m), 1)[0]


def measure_pillow(si, idx, augs, reps, warmup):
    try:
        import PIL  # noqa: F401
    except ImportError:
        return "not measured"
    _, recipe, _, hw, out_hw = SHAPES[si]
    times = []
    with multiprocessing.get_context("spawn").Pool(16, initializer=_worker_init, initargs=(si, hw)) as pool:
        for k in range(warmup + reps):
            jobs = [(int(i), recipe, tuple(int(v) for v in a), out_hw) for i, a in zip(idx, augs[k % len(augs)])]
            t = time.perf_counter()
            batch = np.stack(pool.map(_pillow_one, jobs, chunksize=len(jobs) // 16))
            if k >= warmup:
                times.append((time.perf_counter() - t) * 1e6)
        assert batch.shape == (len(idx), 4) + out_hw
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", choices=["all", "ours"], default="all")
    ap.add_argument("--shapes", default="0,1", help="indices into SHAPES")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [int(s) for s in a.shapes.split(",")]
    IB = importlib.import_module("3d-magic-mirror_amd.input_batches")
    plan = {}
    for si in shapes:
        _, recipe, B, hw, _ = SHAPES[si]
        rng = random.Random(si)
        idx = np.array([rng.randrange(POOL) for _ in range(B)])
        augs = [IB.draw_augmentation(recipe, [hw] * B, rng) for _ in range(4)]
        plan[si] = (idx, augs, measure_pillow(si, idx, augs, a.reps, a.warmup) if a.only == "all" else "not measured")

    import torch                                                      # the GPU is opened only now, after the worker processes are gone
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    rows = []
    for si in shapes:
        name, recipe, B, hw, out_hw = SHAPES[si]
        idx, augs, pillow_us = plan[si]
        imgs, segs = make_sources(si, hw)
        pool = IB.ImagePool(imgs, segs, dev)
        timgs, tsegs = [torch.from_numpy(i).to(dev) for i in imgs], [torch.from_numpy(s).to(dev) for s in segs]
        ours = lambda k: IB.assemble_batch(pool, idx, out_hw, recipe, augs[k % 4])  # noqa: E731
        eager = lambda k: torch.stack([eager_one(timgs[i], tsegs[i], recipe, [int(v) for v in augs[k % 4][b]], out_hw) for b, i in enumerate(idx)])  # noqa: E731
        impls = [("ours", ours)] + ([("eager", eager)] if a.only == "all" else [])
        for k in range(a.warmup):
            for _, f in impls:
                f(k)
        torch.cuda.synchronize()
        times, walls = {k: [] for k, _ in impls}, {k: [] for k, _ in impls}
        for k in range(a.reps):                                       # alternating: drift hits all alike
            for n, f in impls:
                t = time.perf_counter()
                ev[0].record()
                f(k)
                ev[1].record()
                torch.cuda.synchronize()
                walls[n].append((time.perf_counter() - t) * 1e6)
                times[n].append(ev[0].elapsed_time(ev[1]) * 1e3)
        row = {"shape": name, "recipe": recipe, "B": B, "source_hw": hw, "out_hw": out_hw, "pillow_16_workers_wall_us": pillow_us}
        for n in times:
            row["%s_us" % n], row["%s_wall_us" % n] = float(np.median(times[n])), float(np.median(walls[n]))
        row["ours_images_per_s"] = B / (row["ours_wall_us"] * 1e-6)
        if "eager_us" in row:
            row["eager_over_ours"] = row["eager_us"] / row["ours_us"]
            row["eager_note"] = "not bit-equal to the loader: fp32 taps, no rounding to bytes"
            ref = np.abs(eager(0).cpu().numpy() - ours(0).cpu().numpy())
            row["eager_max_abs_diff"] = float(ref.max())
        if isinstance(pillow_us, float):
            row["pillow_over_ours_wall"] = pillow_us / row["ours_wall_us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/bench_input_batches.py", "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
