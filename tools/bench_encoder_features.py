#!/usr/bin/env python3
"""Time the MI355X template-anchored encoder features (encoder_features.py over csrc/mm_encfeat.hip) against the reference's own torch
composition run in fp32 on the GPU (grid_sample + MMPool + the dense torch.mm with the (V,V) Laplacian + cat), per call, with HIP
events: warm-up first, then the median of repeated runs, ours and theirs alternating.  Not called by bench.py.

    python tools/bench_encoder_features.py --out profiles/encoder_features_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_encoder_features.py --only ours --reps 5   # kernel times

Algorithmic bytes (the least any implementation moves): shape forward = read x + write the (B,3C+3,V) output; shape backward = read x,
three of the four row blocks of the upstream gradient (local, glob, neighbor), write d x.  Camera forward = read x + write (B,2C,2,2);
camera backward = read x and the upstream gradient, write d x.  "copy_frac" = bytes / time over the measured 6.29 TB/s copy rate.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
SHAPES = [(32, 2048, 4, 4, "sphere"), (48, 288, 8, 8, "sphere"), (32, 2048, 4, 2, "sphere"), (32, 2048, 4, 4, "smpl_uv")]


def mmpool(x, shape, p):
    w = torch.sigmoid(p)
    return F.adaptive_max_pool2d(x, shape) * w + F.adaptive_avg_pool2d(x, shape) * (1 - w)


def torch_shape(x, template, lpl, p):
    """model_res.py:318-327 as the reference runs it"""
    B, V = x.shape[0], template.shape[1]
    pos = template.repeat(B, 1, 1).view(B, V, 1, 3).detach()
    local = F.grid_sample(x, pos[:, :, :, 0:2], mode="bilinear", align_corners=True, padding_mode="zeros")
    glob = mmpool(x, (1, 1), p).repeat(1, 1, V, 1)
    nd = torch.mm(local.view(-1, V), lpl).view(B, -1, V, 1)
    return torch.cat((local, glob, nd, pos.permute(0, 3, 1, 2)), dim=1).squeeze(3)


def torch_camera(x, template, p_map, p_local):
    """model_res.py:196-200"""
    B, V = x.shape[0], template.shape[1]
    uv = template.repeat(B, 1, 1).view(B, V, 1, 3)[:, :, :, 0:2].detach()
    local = F.grid_sample(x, uv, mode="bilinear", align_corners=False)
    return torch.cat((mmpool(x, (2, 2), p_map), mmpool(local, (2, 2), p_local)), dim=1)


def load_template(pkg, name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "templates", name + ".npz"))
    v = pkg.template.normalize_template(torch.from_numpy(z["vertices"]), 1).float()
    return v[None], pkg.template.uniform_laplacian(v.shape[0], torch.from_numpy(z["faces"]).long()).float()


def timed(fn, ev):
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", choices=["both", "ours"], default="both")
    ap.add_argument("--shapes", default="0,1,2,3", help="indices into SHAPES")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    pkg = importlib.import_module("3d-magic-mirror_amd")
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for si in [int(s) for s in a.shapes.split(",")]:
        B, C, H, W, tname = SHAPES[si]
        template, lpl = load_template(pkg, tname)
        template, lpl = template.to(dev), lpl.to(dev)
        V = template.shape[1]
        g = torch.Generator(device=dev).manual_seed(si)
        x = torch.randn(B, C, H, W, device=dev, generator=g).requires_grad_()
        p, pm, pl = (torch.tensor([v], device=dev, requires_grad=True) for v in (0.0, 0.3, -0.2))
        gs = torch.randn(B, 3 * C + 3, V, device=dev, generator=g)
        gc = torch.randn(B, 2 * C, 2, 2, device=dev, generator=g)
        xb, hw = 4 * B * C * H * W, H * W
        cases = {
            "shape": (lambda: pkg.shape_features(x, template, lpl, p), lambda: torch_shape(x, template, lpl, p), gs,
                      xb + 4 * B * (3 * C + 3) * V, xb + 4 * B * 3 * C * V + xb),
            "camera": (lambda: pkg.camera_features(x, template, pm, pl), lambda: torch_camera(x, template, pm, pl), gc,
                       xb + 4 * B * 2 * C * 4, xb + 4 * B * 2 * C * 4 + xb),
        }
        for op, (ours, theirs, gout, fwd_bytes, bwd_bytes) in cases.items():
            impls = [("ours", ours)] + ([("torch", theirs)] if a.only == "both" else [])

            def fwd(f):
                with torch.no_grad():
                    f()

            def fwdbwd(f):
                f().backward(gout)

            res = {}
            for mode, run in (("fwd", fwd), ("fwd_bwd", fwdbwd)):
                for _ in range(a.warmup):
                    for _, f in impls:
                        run(f)
                torch.cuda.synchronize()
                times = {k: [] for k, _ in impls}
                for _ in range(a.reps):                              # alternating: drift hits both alike
                    for k, f in impls:
                        x.grad = p.grad = pm.grad = pl.grad = None
                        times[k].append(timed(lambda: run(f), ev))
                for k in times:
                    res["%s_%s_us" % (k, mode)] = float(np.median(times[k]))
            row = {"op": op, "B": B, "C": C, "H": H, "W": W, "V": V, "template": tname,
                   "fwd_bytes": fwd_bytes, "fwd_bwd_bytes": fwd_bytes + bwd_bytes, **res}
            for mode, nbytes in (("fwd", fwd_bytes), ("fwd_bwd", fwd_bytes + bwd_bytes)):
                t = res["ours_%s_us" % mode]
                row["ours_%s_copy_frac" % mode] = nbytes / (t * 1e-6) / COPY_RATE
                if "torch_%s_us" % mode in res:
                    row["speedup_%s" % mode] = res["torch_%s_us" % mode] / t
            rows.append(row)
            print(json.dumps(row), flush=True)
        del x, gs, gc
        torch.cuda.empty_cache()
    out = {"tool": "tools/bench_encoder_features.py", "warmup": a.warmup, "reps": a.reps, "copy_rate_Bps": COPY_RATE,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"encoder_features": [(r["op"], r["B"], r["C"], r["H"], r["W"], r["V"], round(r.get("speedup_fwd", 0), 2),
                                            round(r.get("speedup_fwd_bwd", 0), 2)) for r in rows]}))


if __name__ == "__main__":
    main()
