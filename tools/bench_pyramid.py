#!/usr/bin/env python3
"""Time the MI355X three-level pyramid blend (pyramid.pyramid_frames over csrc/mm_pyramid.hip) against the same composition in eager torch
on the same GPU, per call, with HIP events: warm-up first, then --runs alternating runs of ours and eager in one call, the median and
the range of each.  Not called by bench.py.

    python tools/bench_pyramid.py --out profiles/pyramid_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_pyramid.py --only ours --runs 5 --wall-reps 0      # kernel times

B = 48 frames with the tool/generate_market_test preset (background behind a reflection pad of 16 and resized back; kernel 7 with nine
sigmas drawn per frame: three cascaded blurs each of the mask, the background and the render; the six-term blend; bytes), at Market's
128 x 64 and at 128 x 128.  Three forms:
  "ours"       one launch; the call includes lowering the tables on the host and their one small upload.
  "eager"      the same composition BATCHED in eager torch: reflect pad + F.interpolate of the backgrounds, then per level a reflect pad
               + grouped conv2d with the outer-product kernels (one kernel per frame and plane), the differences, the blend, * 255,
               clamp and .to(uint8).  The Gaussian kernels are built before the clock starts.
  "reference"  what the script does (tool/generate_market_test.py:326-369): the pad and resize once per batch, then the same operations one
               image at a time, nine blurs each, ending in a blocking float .cpu() and the multiply and cast on the host [GaussianBlur and
               Resize restated with F.conv2d / F.interpolate: torchvision is not installed; the kernels are built before the clock
               starts, where GaussianBlur builds one per call].  It synchronises per image, so only its wall time is taken.
"wall" times (perf_counter around a synchronised call, median of --wall-reps) run until the bytes are in host memory: ours and eager end in
ONE .cpu() of bytes.  "beyond_range" says whether ours' slowest run beat eager's fastest.  --kernel-us records kernel times measured
separately (the rocprofv3 line above) and the kernel's share of the call."""
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
SITE = "tool/generate_market_test"


def blur(x, k2):
    """x (n,C,H,W), k2 (C,1,k,k): GaussianBlur's reflect pad + depthwise conv2d"""
    r = k2.shape[-1] // 2
    return F.conv2d(F.pad(x, (r, r, r, r), mode="reflect"), k2, groups=x.shape[1])


def resized_backgrounds(Xa, pad):
    H, W = Xa.shape[-2:]
    return F.interpolate(F.pad(Xa[:, :3], (pad,) * 4, mode="reflect"), size=(H, W), mode="bilinear", align_corners=False)


def blend(m, bg, obj):
    return (bg[3] * (1 - m[3]) + obj[3] * m[3] + (bg[1] - bg[2]) * (1 - m[2]) + (obj[1] - obj[2]) * m[2]
            + (bg[0] - bg[1]) * (1 - m[1]) + (obj[0] - obj[1]) * m[1])


def eager_batched(pred, Xa, bgi, pad, k2):
    """k2[kind][level]: (B,1,k,k) for the mask, (3B,1,k,k) for the colour planes"""
    B, _, H, W = pred.shape
    levels = []
    for kind, v in enumerate((pred[:, 3].reshape(1, B, H, W), resized_backgrounds(Xa, pad)[bgi].reshape(1, 3 * B, H, W), pred[:, :3].reshape(1, 3 * B, H, W))):
        lv = [v]
        for level in range(3):
            lv.append(blur(lv[-1], k2[kind][level]))
        levels.append([x.reshape(B, -1, H, W) for x in lv])
    out = blend(*levels)
    return (out.permute(0, 2, 3, 1) * 255).clamp(0, 255).to(torch.uint8)


def reference_loop(pred, Xa, bgi, pad, k2):
    bg = resized_backgrounds(Xa, pad)
    out = []
    for i in range(pred.shape[0]):
        levels = []
        for kind, v in enumerate((pred[i, 3][None, None], bg[int(bgi[i])][None], pred[i, :3][None])):
            lv = [v]
            for level in range(3):
                kk = k2[kind][level]
                lv.append(blur(lv[-1], kk[i:i + 1] if kind == 0 else kk[3 * i:3 * i + 3]))
            levels.append([x[0] for x in lv])
        image = blend(*levels)
        out.append(np.uint8((image.cpu().numpy().transpose(1, 2, 0) * 255).clip(0, 255)))
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
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of ours and eager")
    ap.add_argument("--reps", type=int, default=20, help="calls per run; a run's time is their mean")
    ap.add_argument("--wall-reps", type=int, default=5)
    ap.add_argument("--only", choices=["both", "ours"], default="both")
    ap.add_argument("--kernel-us", default="", help="shape=us,... kernel times from a separate rocprofv3 run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    pkg = importlib.import_module("3d-magic-mirror_amd")
    P = importlib.import_module("3d-magic-mirror_amd.pyramid")
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
        kw = P.preset(SITE, B, generator=hg)
        pad = kw["bg_pad"]
        bgi = torch.randint(0, B, (B,), generator=hg)
        bgi_dev = bgi.to(dev)
        taps = C.gaussian_taps(kw["blur"][0], kw["blur"][1].reshape(-1)).reshape(B, 3, 3, -1)
        outer = taps[..., :, None] * taps[..., None, :]                                       # (B,3,3,k,k)
        k2 = [[(outer[:, kind, level] if kind == 0 else outer[:, kind, level].repeat_interleave(3, 0))[:, None].contiguous().to(dev)
               for level in range(3)] for kind in range(3)]
        ours = lambda: pkg.pyramid_frames(pred, Xa, bgi, **kw)                                # noqa: E731
        eager = lambda: eager_batched(pred, Xa, bgi_dev, pad, k2)                             # noqa: E731
        reference = lambda: reference_loop(pred, Xa, bgi, pad, k2)                            # noqa: E731
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
        for _ in range(a.runs):                                                               # alternating: drift hits both alike
            for k, f in impls:
                times[k].append(float(np.mean([timed(f, ev) for _ in range(a.reps)])))
        row = {"shape": name, "site": SITE, "B": B, "H": H, "W": W}
        for k in times:
            row["%s_us" % k] = float(np.median(times[k]))
            row["%s_min_us" % k], row["%s_max_us" % k] = float(np.min(times[k])), float(np.max(times[k]))
            row["%s_runs_us" % k] = times[k]
        if "eager_us" in row:
            row["speedup"] = row["eager_us"] / row["ours_us"]
            row["beyond_range"] = bool(row["ours_max_us"] < row["eager_min_us"])
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
                row["%s_to_host_wall_min_us" % k], row["%s_to_host_wall_max_us" % k] = float(np.min(wt[k])), float(np.max(wt[k]))
            if "reference_to_host_wall_us" in row:
                row["speedup_to_host_wall_vs_eager"] = row["eager_to_host_wall_us"] / row["ours_to_host_wall_us"]
                row["speedup_to_host_wall_vs_reference"] = row["reference_to_host_wall_us"] / row["ours_to_host_wall_us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/bench_pyramid.py", "warmup": a.warmup, "runs": a.runs, "reps": a.reps, "wall_reps": a.wall_reps,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"pyramid": [(r["shape"], round(r.get("speedup", 0), 2), r.get("beyond_range"),
                                  round(r.get("speedup_to_host_wall_vs_reference", 0), 2)) for r in rows]}))


if __name__ == "__main__":
    main()
