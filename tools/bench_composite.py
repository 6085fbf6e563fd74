#!/usr/bin/env python3
"""Time the MI355X composite of renders over blurred backgrounds (composite.composite_frames over csrc/mm_composite.hip) against the same
composition in eager torch on the same GPU, per call, with HIP events: warm-up first, then the median of repeated runs, ours and eager
alternating in one call.  Not called by bench.py.

    python tools/bench_composite.py --out profiles/composite_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_composite.py --only ours --reps 5 --wall-reps 0      # kernel times

B = 48 frames with the generate_market++ preset (hole fill, mask blur 5 / sigma 3, replicate pad 3 + resize, background behind a
reflection pad (8,8,16,16), blur 5 with one sigma per frame, resize, blend, bytes), at Market's 128 x 64 and at 128 x 128.  Three forms:
  "ours"       one launch; the call includes lowering the tables on the host and their one small upload.
  "eager"      the same composition BATCHED in eager torch: avg_pool2d + two masked assignments, reflect pad + conv2d with the outer-product
               kernel (grouped, one kernel per frame for the background), replicate pad, F.interpolate, the blend, * 255 and .to(uint8).
               The Gaussian kernels are built before the clock starts.
  "reference"  what the scripts do (generate_market++.py:338-349): the same operations one image at a time, each ending in a blocking float
               .cpu() and the multiply and cast on the host [GaussianBlur and Resize restated with F.conv2d / F.interpolate: torchvision is not
               installed].  It synchronises per image, so only its wall time is taken.
"wall" times (perf_counter around a synchronised call, median of --wall-reps) run until the bytes are in host memory: ours and eager end in
ONE .cpu() of bytes.  "spread" is max - min of the event times of that same call; "beyond_spread" says whether ours' slowest run beat
eager's fastest.  --kernel-us records kernel times measured separately (the rocprofv3 line above) and the kernel's share of the call."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("market", 48, 128, 64), ("config2", 48, 128, 128)]
SITE = "generate_market++"


def makeup_hole(mask):
    mask = F.avg_pool2d(mask, 3, stride=1, padding=1)
    mask[mask > 0.7] = 1
    mask[mask <= 0.7] = 0
    return mask


def blur(x, k2):
    """x (n,C,H,W), k2 (C,1,k,k) or (1,1,k,k): GaussianBlur's reflect pad + depthwise conv2d"""
    r = k2.shape[-1] // 2
    return F.conv2d(F.pad(x, (r, r, r, r), mode="reflect"), k2.expand(x.shape[1], 1, -1, -1), groups=x.shape[1])


def eager_batched(pred, Xa, bgi, kw, k_mask, k_bg):
    B, _, H, W = pred.shape
    m = makeup_hole(pred[:, 3:4].clone()) if kw["fill_holes"] else pred[:, 3:4]
    m = blur(m, k_mask)
    p = kw["mask_pad"]
    if p:
        m = F.interpolate(F.pad(m, (p, p, p, p), mode="replicate"), size=(H, W), mode="bilinear", align_corners=False)
    bg = F.pad(Xa[bgi, :3], kw["bg_pad"], mode="reflect")
    bg = blur(bg.reshape(1, B * 3, bg.shape[2], bg.shape[3]), k_bg).reshape(B, 3, bg.shape[2], bg.shape[3])    # one kernel per frame
    bg = F.interpolate(bg, size=(H, W), mode="bilinear", align_corners=False)
    out = pred[:, :3] * m + bg * (1 - m)
    return (out.permute(0, 2, 3, 1) * 255).to(torch.uint8)


def reference_loop(pred, Xa, bgi, kw, k_mask, k_bg):
    H, W = pred.shape[-2:]
    bg = F.pad(Xa[:, :3], kw["bg_pad"], mode="reflect")
    p = kw["mask_pad"]
    out = []
    for i in range(pred.shape[0]):
        single_mask = pred[i, 3][None, None]
        if kw["fill_holes"]:
            single_mask = makeup_hole(single_mask.clone())
        blur_mask = blur(single_mask, k_mask)
        if p:
            blur_mask = F.interpolate(F.pad(blur_mask, (p, p, p, p), mode="replicate"), size=(H, W), mode="bilinear", align_corners=False)
        blur_bg = F.interpolate(blur(bg[int(bgi[i])][None], k_bg[3 * i:3 * i + 3]), size=(H, W), mode="bilinear", align_corners=False)
        image = pred[i, :3] * blur_mask[0] + blur_bg[0] * (1 - blur_mask[0])
        out.append(np.uint8(image.cpu().numpy().transpose(1, 2, 0) * 255))
    return out


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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--wall-reps", type=int, default=5)
    ap.add_argument("--only", choices=["both", "ours"], default="both")
    ap.add_argument("--kernel-us", default="", help="shape=us,... kernel times from a separate rocprofv3 run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    pkg = importlib.import_module("3d-magic-mirror_amd")
    C = importlib.import_module("3d-magic-mirror_amd.composite")
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kernel_us = {k: float(v) for k, v in (kv.split("=") for kv in a.kernel_us.split(",") if kv)}
    rows = []
    for si, (name, B, H, W) in enumerate(SHAPES):
        g = torch.Generator(device=dev).manual_seed(si)
        pred = torch.rand((B, H, W, 4), generator=g, device=dev).movedim(-1, -3)             # NHWC memory, like a render
        pred[:, 3] = (pred[:, 3] * 2 - 0.5).clamp(0, 1)
        Xa = torch.rand((B, 4, H, W), generator=g, device=dev)
        hg = torch.Generator().manual_seed(si)
        kw = C.preset(SITE, B, generator=hg)
        bgi = torch.randint(0, B, (B,), generator=hg)
        bgi_dev = bgi.to(dev)
        t_mask = C.gaussian_taps(*kw["mask_blur"])
        t_bg = C.gaussian_taps(*kw["bg_blur"])
        k_mask = torch.outer(t_mask, t_mask)[None, None].to(dev)
        k_bg = (t_bg[:, :, None] * t_bg[:, None, :]).repeat_interleave(3, 0)[:, None].contiguous().to(dev)   # (3B,1,k,k)
        ours = lambda: pkg.composite_frames(pred, Xa, bgi, **kw)                              # noqa: E731
        eager = lambda: eager_batched(pred, Xa, bgi_dev, kw, k_mask, k_bg)                    # noqa: E731
        reference = lambda: reference_loop(pred, Xa, bgi, kw, k_mask, k_bg)                   # noqa: E731
        if a.only == "both":                                                                  # the three forms make the same frames
            x, y = ours().cpu().int(), eager().cpu().int()
            z = torch.from_numpy(np.stack(reference())).int()
            diff = {"eager": int((x - y).abs().max()), "reference": int((x - z).abs().max())}
            assert max(diff.values()) <= 1, diff
        impls = [("ours", ours)] + ([("eager", eager)] if a.only == "both" else [])
        for _ in range(a.warmup):
            for _, f in impls:
                f()
        torch.cuda.synchronize()
        times = {k: [] for k, _ in impls}
        for _ in range(a.reps):                                                               # alternating: drift hits both alike
            for k, f in impls:
                times[k].append(timed(f, ev))
        row = {"shape": name, "site": SITE, "B": B, "H": H, "W": W}
        for k in times:
            row["%s_us" % k] = float(np.median(times[k]))
            row["%s_min_us" % k], row["%s_max_us" % k] = float(np.min(times[k])), float(np.max(times[k]))
            row["%s_spread_us" % k] = row["%s_max_us" % k] - row["%s_min_us" % k]
        if "eager_us" in row:
            row["speedup"] = row["eager_us"] / row["ours_us"]
            row["beyond_spread"] = bool(row["ours_max_us"] < row["eager_min_us"])
            row["max_byte_difference"] = diff
        if name in kernel_us:
            row["kernel_us"] = kernel_us[name]
            row["kernel_share_of_call"] = kernel_us[name] / row["ours_us"]
        if a.wall_reps:
            walls = [("ours", lambda: ours().cpu())] + ([("eager", lambda: eager().cpu()), ("reference", reference)] if a.only == "both" else [])
            wt = {k: [] for k, _ in walls}
            for _ in range(a.wall_reps):
                for k, f in walls:
                    wt[k].append(wall(f))
            for k in wt:
                row["%s_to_host_wall_us" % k] = float(np.median(wt[k]))
            if "reference_to_host_wall_us" in row:
                row["speedup_to_host_wall_vs_eager"] = row["eager_to_host_wall_us"] / row["ours_to_host_wall_us"]
                row["speedup_to_host_wall_vs_reference"] = row["reference_to_host_wall_us"] / row["ours_to_host_wall_us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/bench_composite.py", "warmup": a.warmup, "reps": a.reps, "wall_reps": a.wall_reps,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"composite": [(r["shape"], round(r.get("speedup", 0), 2), r.get("beyond_spread"),
                                    round(r.get("speedup_to_host_wall_vs_reference", 0), 2)) for r in rows]}))


if __name__ == "__main__":
    main()
