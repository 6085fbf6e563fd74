#!/usr/bin/env python3
"""Time the MI355X PNG encoder (png.encode_png over csrc/mm_png.hip) against Pillow, by the wall clock from frames in device memory to the
files in host memory: warm-up first, then --runs alternating runs of --reps calls each, the median and the range of each form.  Not called
by bench.py.

    python tools/bench_png.py --out profiles/png_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_png.py --only ours --shape config2 --runs 2      # kernel times, a run per shape

The sheets of tools/bench_gif.py: 36 views of B = 48 samples (the sphere template, synthetic attributes) rendered by render_views and laid
out by export_grid as 36 contact sheets, at config 2's 128 x 128 (sheets of 782 x 1042) and at Market's 128 x 64 (782 x 530); and one batch
of 48 texture maps of 256 x 128 (a smooth seeded pattern with a little noise, through export_images).  Forms:
  "ours"       encode_png(frames, segment=S) for S in 1024, 2048 and 4096 (PNG_SEGMENT is one of them): one memset, seven launches, two
               device-to-host copies.  The clock stops when the PngBatch is returned: the files are in host memory.
  "pillow"     what a user has without it: frames.cpu().numpy(), then per frame Image.fromarray(f).save(BytesIO, 'PNG'), one process,
               at Pillow's default level
  "pillow_l1"  the same with compress_level=1
The files differ by design (Pillow codes a frame serially with dynamic Huffman codes); the sizes of all forms are recorded next to the
times.  Before anything is timed Pillow reads every one of ours' files back and it must equal the frame.  "bar" says whether ours' slowest
run (at PNG_SEGMENT) is under the faster yardstick's fastest."""
import argparse
import importlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("config2", 48, 128, 1), ("market", 48, 64, 2), ("textures", 48, 128, 1)]       # name, B, image_size, ratio
VIEWS = 36
SEGMENTS = (1024, 2048, 4096)


def pillow_files(frames, **kw):
    """the files Pillow writes of (n,H,W,3) uint8 frames on the host"""
    from PIL import Image
    out = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "PNG", **kw)
        out.append(buf.getvalue())
    return out


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e6          # us


def sheets_of(pkg, torch, dev, si, B, size, ratio):
    dr = pkg.DiffRender(os.path.join(ROOT, "tests", "golden", "templates", "sphere.npz"), size, ratio=ratio)
    H, W = dr.render_height, size
    att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, B, H, W, seed=si)
    at = {k: att[k].to(dev) for k in ("vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases")}
    at["azimuths"] = (-torch.arange(-180, 180, 10, device=dev, dtype=torch.float32)).expand(B, VIEWS).contiguous()
    with torch.no_grad():
        frames, _ = dr.render_views(no_mask=False, **at)
    return pkg.export_grid(frames, rounding="nearest"), H, W                                  # (36,Hg,Wg,3) uint8, on the device


def textures_of(pkg, torch, dev, si, B, size):
    g = torch.Generator(device="cpu").manual_seed(si)
    coarse = torch.rand(B, 3, 16, 8, generator=g)
    tex = torch.nn.functional.interpolate(coarse, size=(2 * size, size), mode="bicubic", align_corners=False).clamp(0, 1)
    tex = (tex + 0.01 * torch.randn(tex.shape, generator=g)).clamp(0, 1)
    return pkg.export_images(tex.to(dev).contiguous(), rounding="nearest"), 2 * size, size    # (48,256,128,3) uint8, on the device


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of every form")
    ap.add_argument("--reps", type=int, default=10, help="calls of ours per run; a run's time is their mean")
    ap.add_argument("--pillow-reps", type=int, default=1, help="calls of each Pillow form per run")
    ap.add_argument("--only", choices=["all", "ours"], default="all")
    ap.add_argument("--shape", choices=[s[0] for s in SHAPES], default=None, help="one shape only (a profiler run per shape)")
    ap.add_argument("--segments", default=",".join(str(s) for s in SEGMENTS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    pkg = importlib.import_module("3d-magic-mirror_amd")
    dev = torch.device("cuda:0")
    segments = [int(s) for s in a.segments.split(",")]
    rows = []
    for si, (name, B, size, ratio) in enumerate(SHAPES):
        if a.shape not in (None, name):
            continue
        frames, H, W = textures_of(pkg, torch, dev, si, B, size) if name == "textures" else sheets_of(pkg, torch, dev, si, B, size, ratio)
        torch.cuda.synchronize()
        impls = [("ours_%d" % s, (lambda s=s: pkg.encode_png(frames, segment=s))) for s in segments]
        sizes = {k: int(f().offsets[-1]) for k, f in impls}
        if a.only == "all":
            from PIL import Image
            host = frames.cpu().numpy()
            for k, f in impls:
                for i, data in enumerate(f()):
                    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), host[i]), "Pillow must read %s's file %d as the frame" % (k, i)
            impls.append(("pillow", lambda: pillow_files(frames.cpu().numpy())))
            impls.append(("pillow_l1", lambda: pillow_files(frames.cpu().numpy(), compress_level=1)))
            for k, f in impls[-2:]:
                sizes[k] = sum(len(d) for d in f())
        for _ in range(a.warmup):
            for k, f in impls:
                if not k.startswith("pillow"):
                    f()
        times = {k: [] for k, _ in impls}
        for _ in range(a.runs):                                                               # alternating: drift hits all alike
            for k, f in impls:
                reps = a.pillow_reps if k.startswith("pillow") else a.reps
                times[k].append(float(np.mean([wall(f) for _ in range(reps)])))
        row = {"shape": name, "B": B, "n": int(frames.shape[0]), "H": H, "W": W, "frame": list(frames.shape[1:3]), "frame_bytes_total": int(frames.numel()),
               "png_segment": pkg.PNG_SEGMENT, "file_bytes": sizes}
        for k in times:
            row["%s_us" % k] = float(np.median(times[k]))
            row["%s_min_us" % k], row["%s_max_us" % k] = float(np.min(times[k])), float(np.max(times[k]))
            row["%s_runs_us" % k] = times[k]
        ours = "ours_%d" % pkg.PNG_SEGMENT
        if "pillow_us" in row and ours + "_us" in row:
            fastest = min(row["pillow_min_us"], row["pillow_l1_min_us"])
            row["speedup_vs_pillow"] = row["pillow_us"] / row[ours + "_us"]
            row["speedup_vs_pillow_l1"] = row["pillow_l1_us"] / row[ours + "_us"]
            row["bar"] = bool(row[ours + "_max_us"] < fastest)
            row["bar_by_segment"] = {str(s): bool(row["ours_%d_max_us" % s] < fastest) for s in segments}
            row["file_bytes_vs_pillow"] = sizes[ours] / sizes["pillow"]
            row["file_bytes_vs_pillow_l1"] = sizes[ours] / sizes["pillow_l1"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/bench_png.py", "warmup": a.warmup, "runs": a.runs, "reps": a.reps, "pillow_reps": a.pillow_reps,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"png": [(r["shape"], round(r.get("speedup_vs_pillow", 0), 2), round(r.get("speedup_vs_pillow_l1", 0), 2), r.get("bar"),
                               round(r.get("file_bytes_vs_pillow", 0), 2)) for r in rows]}))


if __name__ == "__main__":
    main()
