#!/usr/bin/env python3
"""Time the MI355X GIF encoder (gif.encode_gif over csrc/mm_gif.hip) against Pillow, by the wall clock from frames in device memory to the
file in host memory: warm-up first, then --runs alternating runs of --reps calls each, the median and the range of each form.  Not called
by bench.py.

    python tools/bench_gif.py --out profiles/gif_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_gif.py --only ours --shape config2 --runs 2      # kernel times, a run per shape

The turntable of trainer.py:616-631: 36 views of B = 48 samples (the sphere template, synthetic attributes) rendered by render_views and
laid out by export_grid as 36 contact sheets, at config 2's 128 x 128 (sheets of 782 x 1042) and at Market's 128 x 64 (782 x 530).  Forms:
  "ours"     encode_gif(sheets, segment=S) for S in 512, 1024 and 2048 (GIF_SEGMENT is one of them): one memset, eight launches, two
             device-to-host copies.  The clock stops when the GifFile is returned: the file is in host memory.
  "pillow"   what a user has without it: sheets.cpu().numpy(), then Image.fromarray(f) per frame and
             first.save(BytesIO, 'GIF', save_all=True, append_images=rest, duration=100, loop=0), one process.  (imageio, which the reference
             calls, is not installed; it writes GIFs through Pillow.)
The files differ by design (Pillow quantises every frame on its own and codes with one full dictionary); both sizes are recorded next to the
times.  Before anything is timed Pillow reads ours' file back and every frame must be palette[indices] of quantize_frames.  "bar" says
whether ours' slowest run (at GIF_SEGMENT) is under the yardstick's fastest.  --kernel-us records kernel times measured separately (the
rocprofv3 line above: the sum over the kernels and the memset of one call) and their share of the call."""
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

SHAPES = [("config2", 48, 128, 1), ("market", 48, 64, 2)]       # name, B, image_size, ratio
VIEWS = 36
SEGMENTS = (512, 1024, 2048)


def pillow_file(sheets):
    """the file Pillow writes of (n,H,W,3) uint8 frames on the host"""
    from PIL import Image
    ims = [Image.fromarray(f) for f in sheets]
    buf = io.BytesIO()
    ims[0].save(buf, "GIF", save_all=True, append_images=ims[1:], duration=100, loop=0)
    return buf.getvalue()


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e6          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of every form")
    ap.add_argument("--reps", type=int, default=20, help="calls of ours per run; a run's time is their mean")
    ap.add_argument("--pillow-reps", type=int, default=None, help="calls of Pillow per run (default: --reps)")
    ap.add_argument("--only", choices=["all", "ours"], default="all")
    ap.add_argument("--shape", choices=[s[0] for s in SHAPES], default=None, help="one shape only (a profiler run per shape)")
    ap.add_argument("--segments", default=",".join(str(s) for s in SEGMENTS))
    ap.add_argument("--kernel-us", default="", help="shape=us,... device time of one call from a separate rocprofv3 run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    pkg = importlib.import_module("3d-magic-mirror_amd")
    G = importlib.import_module("3d-magic-mirror_amd.gif")
    dev = torch.device("cuda:0")
    segments = [int(s) for s in a.segments.split(",")]
    kernel_us = {k: float(v) for k, v in (kv.split("=") for kv in a.kernel_us.split(",") if kv)}
    rows = []
    for si, (name, B, size, ratio) in enumerate(SHAPES):
        if a.shape not in (None, name):
            continue
        dr = pkg.DiffRender(os.path.join(ROOT, "tests", "golden", "templates", "sphere.npz"), size, ratio=ratio)
        H, W = dr.render_height, size
        att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, B, H, W, seed=si)
        at = {k: att[k].to(dev) for k in ("vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases")}
        at["azimuths"] = (-torch.arange(-180, 180, 10, device=dev, dtype=torch.float32)).expand(B, VIEWS).contiguous()
        with torch.no_grad():
            frames, _ = dr.render_views(no_mask=False, **at)
        sheets = pkg.export_grid(frames)                                                      # (36,Hg,Wg,3) uint8, on the device
        del frames
        torch.cuda.synchronize()
        impls = [("ours_%d" % s, (lambda s=s: pkg.encode_gif(sheets, segment=s))) for s in segments]
        sizes = {k: len(f()) for k, f in impls}
        if a.only == "all":
            from PIL import Image
            pal, idx = (t.cpu().numpy() for t in pkg.quantize_frames(sheets))
            im = Image.open(io.BytesIO(bytes(impls[0][1]())))
            assert im.n_frames == VIEWS
            for i in range(VIEWS):
                im.seek(i)
                assert np.array_equal(np.asarray(im.convert("RGB")), pal[idx[i]]), "Pillow must read ours' frame %d as palette[indices]" % i
            impls.append(("pillow", lambda: pillow_file(sheets.cpu().numpy())))
            sizes["pillow"] = len(impls[-1][1]())
        for _ in range(a.warmup):
            for k, f in impls:
                if k != "pillow":
                    f()
        times = {k: [] for k, _ in impls}
        for _ in range(a.runs):                                                               # alternating: drift hits all alike
            for k, f in impls:
                reps = (a.pillow_reps or a.reps) if k == "pillow" else a.reps
                times[k].append(float(np.mean([wall(f) for _ in range(reps)])))
        row = {"shape": name, "B": B, "views": VIEWS, "H": H, "W": W, "sheet": list(sheets.shape[1:3]), "frame_bytes_total": int(sheets.numel()),
               "gif_segment": G.GIF_SEGMENT, "file_bytes": sizes}
        for k in times:
            row["%s_us" % k] = float(np.median(times[k]))
            row["%s_min_us" % k], row["%s_max_us" % k] = float(np.min(times[k])), float(np.max(times[k]))
            row["%s_runs_us" % k] = times[k]
        ours = "ours_%d" % G.GIF_SEGMENT
        if "pillow_us" in row and ours + "_us" in row:
            row["speedup_vs_pillow"] = row["pillow_us"] / row[ours + "_us"]
            row["bar"] = bool(row[ours + "_max_us"] < row["pillow_min_us"])
            row["file_bytes_vs_pillow"] = sizes[ours] / sizes["pillow"]
        if name in kernel_us and ours + "_us" in row:
            row["device_us"] = kernel_us[name]
            row["device_share_of_call"] = kernel_us[name] / row[ours + "_us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/bench_gif.py", "warmup": a.warmup, "runs": a.runs, "reps": a.reps, "pillow_reps": a.pillow_reps or a.reps,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"gif": [(r["shape"], round(r.get("speedup_vs_pillow", 0), 2), r.get("bar"), round(r.get("file_bytes_vs_pillow", 0), 2)) for r in rows]}))


if __name__ == "__main__":
    main()
