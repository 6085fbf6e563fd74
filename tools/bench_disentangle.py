#!/usr/bin/env python3
"""Time the MI355X disentangle regularisation (disentangle.py over csrc/mm_disentangle.hip) against the reference's own composition
(trainer.py:455-494 with smr_utils.fliplr and RandomErasing's clone + slice write) restated in eager fp32 torch on the same device, with
HIP events: warm-up first, then five runs of twenty calls each, ours and eager alternating; median and range of the per-call time.  Not
called by bench.py.

    python tools/bench_disentangle.py --out profiles/disentangle_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_disentangle.py --only ours --runs 1       # kernel times
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_disentangle.py --probe PART               # what the forward kernel's time is made of

``--probe`` launches nothing but 30 forwards of ``disentangle_terms`` at config 2, one rocprofv3 run per PART, so that the trace's
``dis_fwd_kernel`` row is that part alone: ``full`` (both sets), ``v1`` (both sets with V = 1: the texture stream, the camera sums and the
last-workgroup fold, next to no per-sample sums), ``flip`` (the flipped set alone: the stream and one per-sample sum per sample),
``jitter`` (the erased set alone: no stream; the per-sample sums, the camera sums and the fold).

Three comparisons per shape: "inputs" (the two encoder batches from Xa), "fwd" (the seven terms under no_grad) and "fwd_bwd" (the terms
composed with dis1 = dis2 = 1, then backward into all fourteen leaves).  Algorithmic bytes: inputs read 4 BCHW and write 8 BCHW; the
terms' forward reads the two textures (2 * 12 B Ht Wt) and four (B,V,3) arrays; the backward reads the same and writes two texture
gradients and four (B,V,3) gradients.  "copy_frac" = bytes / time over the measured 6.29 TB/s device-to-device copy rate -- of the CALL
here (host time and launches included); the kernels' own times come from the rocprofv3 run."""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
SHAPES = [("config2", 48, 128, 128, 642, 256, 128), ("market", 48, 128, 64, 642, 256, 64)]        # name, B, H, W, V, Ht, Wt
BASE = ("textures", "vertices", "azimuths", "elevations", "distances", "biases", "delta_vertices")


def mirrored(x):
    """the columns reversed the eager way the reference takes: an index_select on an index built for the call (not ``flip``)"""
    return x.index_select(3, torch.arange(x.shape[3] - 1, -1, -1, device=x.device))


def unit_circle(degrees):
    r = degrees * math.pi / 180.0
    return torch.stack([torch.cos(r), torch.sin(r)], 1)


def eager_inputs(Xa, box):
    i, j, h, w = box
    erased = Xa.clone()
    erased[..., i:i + h, j:j + w] = 0.0
    return mirrored(Xa), erased


def mean_row_norm(a, b):
    return torch.norm((a - b).flatten(1), p=2, dim=1).mean()


def mean_square(a, b):
    return (a - b).pow(2).mean()


def eager_block(Ae, Af, Aj, dis1=1.0, dis2=1.0, azim=1.0):
    """the seven terms composed as eager torch composes them, operation for operation what the reference's block launches"""
    x_negated = Ae["vertices"].clone()
    x_negated[..., 0] *= -1
    flip_half = (mirrored(Af["textures"]) - Ae["textures"]).abs().mean() + mean_row_norm(Af["vertices"], x_negated)
    camera = (azim * mean_square(unit_circle(Aj["azimuths"]), unit_circle(Ae["azimuths"]))
              + mean_square(unit_circle(Aj["elevations"]), unit_circle(Ae["elevations"]))
              + mean_square(Aj["distances"], Ae["distances"]) + mean_square(Aj["biases"], Ae["biases"]))
    return dis1 * flip_half + dis2 * (camera + mean_row_norm(Aj["delta_vertices"], Ae["delta_vertices"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", choices=["both", "ours"], default="both")
    ap.add_argument("--out", default=None)
    ap.add_argument("--probe", choices=["full", "v1", "flip", "jitter"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    pkg = importlib.import_module("3d-magic-mirror_amd")
    dev = torch.device("cuda:0")
    if a.probe:
        return probe(pkg, dev, a.probe)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dr = _any_renderer(pkg)
    rows = []
    for si, (name, B, H, W, V, Ht, Wt) in enumerate(SHAPES):
        g = torch.Generator(device=dev).manual_seed(si)
        r = lambda *s: torch.rand(*s, generator=g, device=dev)  # noqa: E731
        Xa = r(B, 4, H, W)
        box = (H // 4, W // 4, H // 3, W // 2)

        def one():
            return {"textures": r(B, 3, Ht, Wt), "vertices": r(B, V, 3) - 0.5, "azimuths": r(B) * 360 - 180, "elevations": r(B) * 30,
                    "distances": r(B) * 5 + 2, "biases": r(B, 2) * 0.6 - 0.3, "delta_vertices": (r(B, V, 3) - 0.5) * 0.2}
        sets = [{k: v.requires_grad_(True) for k, v in one().items()} for _ in range(3)]
        Ae, Af, Aj = sets
        Af = {k: Af[k] for k in ("textures", "vertices")}
        Aj = {k: Aj[k] for k in BASE[2:]}
        leaves = list(Ae.values()) + list(Af.values()) + list(Aj.values())

        def ours_terms():
            return dr.recon_disentangle(Ae, Af, Aj, 1.0, 1.0)

        def no_grad(f):
            def run():
                with torch.no_grad():
                    f()
            return run

        def with_backward(f):
            def run():
                for t in leaves:
                    t.grad = None
                f().backward()
            return run

        modes = {"inputs": (lambda: pkg.disentangle_inputs(Xa, box), lambda: eager_inputs(Xa, box)),
                 "fwd": (no_grad(ours_terms), no_grad(lambda: eager_block(Ae, Af, Aj))),
                 "fwd_bwd": (with_backward(ours_terms), with_backward(lambda: eager_block(Ae, Af, Aj)))}
        tex, mesh = 12 * B * Ht * Wt, 12 * B * V
        nbytes = {"inputs": 3 * 16 * B * H * W, "fwd": 2 * tex + 4 * mesh, "fwd_bwd": 2 * (2 * tex + 4 * mesh) + 2 * tex + 4 * mesh}
        row = {"shape": name, "B": B, "H": H, "W": W, "V": V, "Ht": Ht, "Wt": Wt, "calls_per_run": a.calls, "runs": a.runs}
        for mode, (ours, eager) in modes.items():
            impls = [("ours", ours)] + ([("eager", eager)] if a.only == "both" else [])
            for _ in range(a.warmup):
                for _, f in impls:
                    f()
            torch.cuda.synchronize()
            times = {k: [] for k, _ in impls}
            for _ in range(a.runs):                                 # alternating: drift hits both alike
                for k, f in impls:
                    ev[0].record()
                    for _ in range(a.calls):
                        f()
                    ev[1].record()
                    torch.cuda.synchronize()
                    times[k].append(ev[0].elapsed_time(ev[1]) * 1e3 / a.calls)          # us per call
            for k, t in times.items():
                row["%s_%s_us" % (k, mode)] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}
            row["%s_bytes" % mode] = nbytes[mode]
            row["ours_%s_copy_frac" % mode] = nbytes[mode] / (row["ours_%s_us" % mode]["median"] * 1e-6) / COPY_RATE
            if "eager" in times:
                row["speedup_%s" % mode] = row["eager_%s_us" % mode]["median"] / row["ours_%s_us" % mode]["median"]
                row["ours_slowest_under_eager_fastest_%s" % mode] = bool(max(times["ours"]) < min(times["eager"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/bench_disentangle.py", "warmup": a.warmup, "runs": a.runs, "calls": a.calls, "copy_rate_Bps": COPY_RATE,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def probe(pkg, dev, part, calls=30):
    """30 forwards of the terms at config 2 and nothing else on the device but their set-up: for a kernel trace (module docstring)"""
    _, B, _, _, V, Ht, Wt = SHAPES[0]
    V = 1 if part == "v1" else V
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g, device=dev)  # noqa: E731
    sets = [{"textures": r(B, 3, Ht, Wt), "vertices": r(B, V, 3) - 0.5, "azimuths": r(B) * 360 - 180, "elevations": r(B) * 30,
             "distances": r(B) * 5 + 2, "biases": r(B, 2) * 0.6 - 0.3, "delta_vertices": (r(B, V, 3) - 0.5) * 0.2} for _ in range(3)]
    Ae, Af, Aj = sets[0], (None if part == "jitter" else sets[1]), (None if part == "flip" else sets[2])
    with torch.no_grad():
        for _ in range(calls):
            pkg.disentangle_terms(Ae, Af, Aj)
    torch.cuda.synchronize()
    print(json.dumps({"probe": part, "B": B, "V": V, "Ht": Ht, "Wt": Wt, "calls": calls}))


def _any_renderer(pkg):
    """recon_disentangle reads nothing of the renderer: any DiffRender serves (the sphere template, as the tests use)"""
    return pkg.DiffRender(os.path.join(ROOT, "tests", "golden", "templates", "sphere.npz"), 32)


if __name__ == "__main__":
    main()
