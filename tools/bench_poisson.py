#!/usr/bin/env python3
"""Time the MI355X Poisson blend (poisson.poisson_frames over csrc/mm_poisson.hip) per call, with HIP events and by the wall clock until
the bytes are on the host: warm-up first, then --runs alternating runs of ours and the eager form in one call, the median and the range
of each.  Not called by bench.py.

    python tools/bench_poisson.py --out profiles/poisson_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_poisson.py --only ours --runs 5 --wall-reps 0      # kernel times
    python tools/bench_poisson.py --only ours --lib <a library built with -DMM_POISSON_BLOCK=256>                       # workgroup size

B = 48 frames with the tool/generate_market_test preset (background behind a reflection pad of 16 and resized back), the mask from the
render's alpha, border "reference", the default sweeps and omega, at Market's 128 x 64 and at 128 x 128.  Three forms:
  "ours"   one launch; the call includes lowering the tables on the host and their one small upload.
  "eager"  the same red-black SOR order composed from eager torch operators on the GPU, batched over frames and channels: the padded
           resize of the backgrounds, the right-hand side, then per half-sweep a zero pad, four shifted views, the update and a where.
  "host"   the route the reference offers (poisson_image_editing.py): the float frames copied to the host, then the system assembled
           once per frame and one sparse direct solve (scipy.sparse.linalg.spsolve) per frame and channel, in one process, fp64.  Wall
           time only.
"beyond_range" says whether ours' slowest run beat the yardstick's fastest."""
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


def targets(Xa, pad):
    H, W = Xa.shape[-2:]
    return F.interpolate(F.pad(Xa[:, :3], (pad,) * 4, mode="reflect"), size=(H, W), mode="bilinear", align_corners=False)


def shifted(v):
    z = F.pad(v, (1, 1, 1, 1))
    return z[..., 1:-1, :-2], z[..., 1:-1, 2:], z[..., :-2, 1:-1], z[..., 2:, 1:-1]


def eager_batched(pred, Xa, bgi, pad, sweeps, omega, colours, edge):
    s, t = pred[:, :3], targets(Xa, pad)[bgi]
    inside = ((pred[:, 3:] * 255).clamp(0, 255).to(torch.uint8) != 0).expand_as(s)
    l, r, u, d = shifted(s)
    b = torch.where(inside, 4.0 * s - ((l + r) + (u + d)), t)
    free = inside | edge
    x = t.clone()
    for _ in range(sweeps):
        for colour in colours:
            l, r, u, d = shifted(x)
            x = torch.where(free & colour, x + omega * (((b + ((l + r) + (u + d))) * 0.25) - x), x)
    return (x.permute(0, 2, 3, 1) * 255).clamp(0, 255).to(torch.uint8)


def host_direct(pred, Xa, bgi, pad):
    """frames to the host, one spsolve per frame and channel"""
    import scipy.sparse
    from scipy.sparse.linalg import spsolve
    s_all, t_all, a_all = pred[:, :3].cpu().double().numpy(), targets(Xa, pad)[bgi].cpu().double().numpy(), pred[:, 3].cpu().numpy()
    B, _, H, W = s_all.shape
    idx = np.arange(H * W).reshape(H, W)
    edge = np.zeros((H, W), dtype=bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    out = np.empty((B, H, W, 3), dtype=np.uint8)
    for i in range(B):
        inside = np.uint8(np.clip(a_all[i] * 255, 0, 255)) != 0
        free = inside | edge
        rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.where(free, 4.0, 1.0).ravel()]
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            ok = free.copy()
            ok[:max(-dy, 0)] = False; ok[H - max(dy, 0):] = False; ok[:, :max(-dx, 0)] = False; ok[:, W - max(dx, 0):] = False
            rows.append(idx[ok]); cols.append(idx[ok] + dy * W + dx); vals.append(np.full(int(ok.sum()), -1.0))
        A = scipy.sparse.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W))
        for c in range(3):
            z = np.pad(s_all[i, c], 1)
            lap = 4.0 * s_all[i, c] - (z[1:-1, :-2] + z[1:-1, 2:] + z[:-2, 1:-1] + z[2:, 1:-1])
            x = spsolve(A, np.where(inside, lap, t_all[i, c]).ravel()).reshape(H, W)
            out[i, :, :, c] = np.uint8(np.clip(x * 255, 0, 255))
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of ours and eager")
    ap.add_argument("--reps", type=int, default=20, help="calls of ours per run; a run's time is their mean")
    ap.add_argument("--eager-reps", type=int, default=20, help="calls of the eager form per run (each is some ten thousand launches)")
    ap.add_argument("--wall-reps", type=int, default=3)
    ap.add_argument("--only", choices=["both", "ours"], default="both")
    ap.add_argument("--lib", default=None, help="load this build of libmm_render.so (another MM_POISSON_BLOCK) instead of the package's")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    if a.lib:
        importlib.import_module("3d-magic-mirror_amd._native").LIB_PATH = os.path.abspath(a.lib)
    P = importlib.import_module("3d-magic-mirror_amd.poisson")
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for si, (name, B, H, W) in enumerate(SHAPES):
        g = torch.Generator(device=dev).manual_seed(si)
        pred = torch.rand((B, H, W, 4), generator=g, device=dev).movedim(-1, -3)             # NHWC memory, like a render
        pred[:, 3] = (pred[:, 3] * 2 - 0.5).clamp(0, 1)
        Xa = torch.rand((B, 4, H, W), generator=g, device=dev)
        kw = P.PRESETS[SITE]
        bgi = torch.randint(0, B, (B,), generator=torch.Generator().manual_seed(si))
        bgi_dev = bgi.to(dev)
        sweeps, omega = P.default_sweeps(H, W), torch.tensor(P.default_omega(H, W), device=dev)
        even = ((torch.arange(H, device=dev)[:, None] + torch.arange(W, device=dev)[None]) % 2 == 0)
        edge = torch.zeros((H, W), dtype=torch.bool, device=dev)
        edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
        ours = lambda: P.poisson_frames(pred, Xa, bgi, **kw)                                  # noqa: E731
        eager = lambda: eager_batched(pred, Xa, bgi_dev, kw["bg_pad"], sweeps, omega, (even, ~even), edge)   # noqa: E731
        host = lambda: host_direct(pred, Xa, bgi_dev, kw["bg_pad"])                           # noqa: E731
        row = {"shape": name, "site": SITE, "B": B, "H": H, "W": W, "sweeps": sweeps, "omega": float(omega), "lib": a.lib}
        if a.only == "both":                                                                  # the three forms make the same frames
            x, y, z = ours().cpu().int(), eager().cpu().int(), torch.from_numpy(host()).int()
            row["max_byte_difference"] = {"eager": int((x - y).abs().max()), "host": int((x - z).abs().max())}
            row["bytes_that_differ"] = {"eager": int((x != y).sum()), "host": int((x != z).sum())}
            assert max(row["max_byte_difference"].values()) <= 1, row
        impls = [("ours", ours, a.reps)] + ([("eager", eager, a.eager_reps)] if a.only == "both" else [])
        for _ in range(a.warmup):
            ours()
        torch.cuda.synchronize()
        times = {k: [] for k, _, _ in impls}
        for _ in range(a.runs):                                                               # alternating: drift hits both alike
            for k, f, reps in impls:
                times[k].append(float(np.mean([timed(f, ev) for _ in range(reps)])))
        for k in times:
            row["%s_us" % k] = float(np.median(times[k]))
            row["%s_min_us" % k], row["%s_max_us" % k] = float(np.min(times[k])), float(np.max(times[k]))
            row["%s_runs_us" % k] = times[k]
        if "eager_us" in row:
            row["speedup_vs_eager"] = row["eager_us"] / row["ours_us"]
            row["beyond_range_vs_eager"] = bool(row["ours_max_us"] < row["eager_min_us"])
        if a.wall_reps:
            walls = [("ours", lambda: ours().cpu())] + ([("eager", lambda: eager().cpu()), ("host", host)] if a.only == "both" else [])
            wt = {k: [] for k, _ in walls}
            for _ in range(a.wall_reps):
                for k, f in walls:
                    wt[k].append(wall(f))
            for k in wt:
                row["%s_to_host_wall_us" % k] = float(np.median(wt[k]))
                row["%s_to_host_wall_min_us" % k], row["%s_to_host_wall_max_us" % k] = float(np.min(wt[k])), float(np.max(wt[k]))
            if "host_to_host_wall_us" in row:
                row["speedup_to_host_wall_vs_eager"] = row["eager_to_host_wall_us"] / row["ours_to_host_wall_us"]
                row["speedup_to_host_wall_vs_host"] = row["host_to_host_wall_us"] / row["ours_to_host_wall_us"]
                row["beyond_range_to_host_wall_vs_eager"] = bool(row["ours_to_host_wall_max_us"] < row["eager_to_host_wall_min_us"])
                row["beyond_range_to_host_wall_vs_host"] = bool(row["ours_to_host_wall_max_us"] < row["host_to_host_wall_min_us"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/bench_poisson.py", "warmup": a.warmup, "runs": a.runs, "reps": a.reps, "eager_reps": a.eager_reps,
           "wall_reps": a.wall_reps, "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"poisson": [(r["shape"], round(r["ours_us"], 1), round(r.get("speedup_vs_eager", 0), 1),
                                  round(r.get("speedup_to_host_wall_vs_host", 0), 1)) for r in rows]}))


if __name__ == "__main__":
    main()
