#!/usr/bin/env python3
"""Time the MI355X attribute interpolation (interpolate.interpolate_attributes over csrc/mm_interp.hip) against the reference's block
(trainer.py:279-340) restated in eager fp32 torch on the GPU -- with its device-to-host copy of the collapse test and numpy's
resampling -- per call, with HIP events: warm-up first, then the median of repeated runs, ours and eager alternating.  Not called by
bench.py.

    python tools/bench_interpolate.py --out profiles/interpolate_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_interpolate.py --only ours --reps 5 --no-situ   # kernel times

Three timings per shape: "fwd" (the block under no_grad), "fwd_bwd" (the block, then backward of sum(w * Ai) over the five mixed
tensors with fixed random weights w, into Ae's leaves) and "situ" (render #1 -> the block -> render #2 -> recon_data of both ->
backward: where the reference's sync stalls the queue).  Algorithmic bytes: with S the bytes of one attribute set (vertices,
delta_vertices, textures, bg, lights in fp32), the mix reads two rows and writes one (3 S) forward and reads the upstream gradient
and writes the source gradient (2 S) backward.  "copy_frac" = bytes / time over the measured 6.29 TB/s copy rate.
"""
import argparse
import importlib
import json
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
# name, B, V, Ht, Wt, image side (bg is image side squared)
SHAPES = [("config2", 48, 642, 256, 128, 128), ("config3", 48, 642, 512, 256, 256), ("config2x8", 384, 642, 256, 128, 128)]
OPT = types.SimpleNamespace(hard=True, hard_range=20, inv=0, lambda_ic=0.1, azi_scope=360, bias_range=0.5, beta=0.0, bg=True)
ELEV, DIST = (0.0, 30.0), (2.0, 7.0)
MIX = ("vertices", "delta_vertices", "textures", "bg", "lights")


def eager_block(Ae, opt, deep_copy):
    """trainer.py:279-340 as the reference runs it, in fp32 on the device"""
    B, dev = Ae["vertices"].shape[0], Ae["vertices"].device
    f32 = dict(dtype=torch.float32, device=dev)
    Ae90 = None
    if opt.hard:
        Ae90 = deep_copy(Ae)
        if random.random() > 0.5:
            Ae90["azimuths"] = -torch.empty(B, **f32).uniform_(opt.hard_range, 180 - opt.hard_range)
        else:
            Ae90["azimuths"] = -torch.empty(B, **f32).uniform_(0, 180)
        rand = torch.empty(B, **f32).uniform_(-1.0, 1.0)
        rand[rand < 0] = -1.0
        rand[rand >= 0] = 1.0
        Ae90["azimuths"] *= rand
    mean_delta = torch.mean(torch.abs(Ae["delta_vertices"])[:, -1], dim=1)
    bad_index = np.argwhere(mean_delta.data.cpu().numpy() > 0.4)
    rand_a, rand_b = np.random.permutation(B), np.random.permutation(B)
    if opt.inv == 0:
        good_index = np.setdiff1d(np.arange(B), bad_index)
        for i in bad_index:
            rand_a[np.argwhere(rand_a == i)] = np.random.choice(good_index, 1)
            rand_b[np.argwhere(rand_b == i)] = np.random.choice(good_index, 1)
    Aa, Ab = deep_copy(Ae, torch.LongTensor(rand_a)), deep_copy(Ae, torch.LongTensor(rand_b))
    Ai = {}
    torch.empty(B, **f32).uniform_(0.0, 1.0)
    Ai["azimuths"] = -torch.empty(B, **f32).uniform_(-opt.azi_scope / 2, opt.azi_scope / 2)
    Ai["elevations"] = torch.empty(B, **f32).uniform_(*ELEV)
    Ai["distances"] = torch.empty(B, **f32).uniform_(*DIST)
    Ai["biases"] = torch.empty((B, 2), **f32).uniform_(-opt.bias_range, opt.bias_range)
    a_t = torch.empty((B, 1, 1, 1), **f32).uniform_(0.0, 1.0)
    a_s = torch.empty((B, 1, 1), **f32).uniform_(0.0, 1.0)
    Ai["vertices"] = a_s * Aa["vertices"] + (1 - a_s) * Ab["vertices"]
    Ai["delta_vertices"] = a_s * Aa["delta_vertices"] + (1 - a_s) * Ab["delta_vertices"]
    Ai["textures"] = a_t * Aa["textures"] + (1.0 - a_t) * Ab["textures"]
    Ai["bg"] = a_t * Aa["bg"] + (1.0 - a_t) * Ab["bg"] if opt.bg else None
    a_l = torch.empty((B, 1), **f32).uniform_(0.0, 1.0)
    Ai["lights"] = a_l * Aa["lights"] + (1.0 - a_l) * Ab["lights"]
    return Ai, Ae90


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
    ap.add_argument("--shapes", default="0,1,2", help="indices into SHAPES")
    ap.add_argument("--no-situ", action="store_true", help="skip the render #1 -> block -> render #2 -> backward sequence")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    pkg = importlib.import_module("3d-magic-mirror_amd")
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for si in [int(s) for s in a.shapes.split(",")]:
        name, B, V, Ht, Wt, S_img = SHAPES[si]
        dr = pkg.DiffRender(os.path.join(ROOT, "tests", "golden", "templates", "smpl_uv_642.npz"), S_img)
        att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, B, Ht // 2, Wt, seed=si)   # textures (B,3,Ht,Wt)
        att["bg"] = torch.rand(B, 3, S_img, S_img)
        gt = torch.nn.functional.interpolate(gt, size=(S_img, S_img)).to(dev)
        leaves = {k: v.to(dev).requires_grad_() for k, v in att.items() if torch.is_tensor(v)}
        assert leaves["textures"].shape == (B, 3, Ht, Wt) and leaves["vertices"].shape == (B, V, 3)
        g = torch.Generator(device=dev).manual_seed(si)
        w = {"vertices": (B, V, 3), "delta_vertices": (B, V, 3), "textures": (B, 3, Ht, Wt), "bg": (B, 3, S_img, S_img), "lights": (B, 9)}
        w = {k: torch.randn(s, generator=g, device=dev) for k, s in w.items()}
        S = 4 * B * (6 * V + 3 * Ht * Wt + 3 * S_img * S_img + 9)

        def ours(Ae):
            return pkg.interpolate_attributes(Ae, OPT, ELEV, DIST)

        def theirs(Ae):
            return eager_block(Ae, OPT, pkg.deep_copy)

        impls = [("ours", ours)] + ([("eager", theirs)] if a.only == "both" else [])

        def fwd(f):
            with torch.no_grad():
                f(dict(leaves))

        def fwdbwd(f):
            Ai, _ = f(dict(leaves))
            sum((Ai[k] * w[k]).sum() for k in MIX).backward()

        def situ(f):
            rgbs_e, Ae = dr.render(no_mask=True, **dict(leaves))
            Ai, _ = f(Ae)
            rgbs_i, _ = dr.render(no_mask=True, **Ai)
            (dr.recon_data(rgbs_e, gt, no_mask=True) + dr.recon_data(rgbs_i, gt, no_mask=True)).backward()

        modes = [("fwd", fwd), ("fwd_bwd", fwdbwd)] + ([] if a.no_situ else [("situ", situ)])
        res = {}
        for mode, run in modes:
            for _ in range(a.warmup):
                for _, f in impls:
                    run(f)
            torch.cuda.synchronize()
            times = {k: [] for k, _ in impls}
            for rep in range(a.reps):                                # alternating: drift hits both alike
                for k, f in impls:
                    for t in leaves.values():
                        t.grad = None
                    random.seed(rep)
                    np.random.seed(rep)
                    times[k].append(timed(lambda: run(f), ev))
            for k in times:
                res["%s_%s_us" % (k, mode)] = float(np.median(times[k]))
        row = {"shape": name, "B": B, "V": V, "Ht": Ht, "Wt": Wt, "H": S_img, "W": S_img, "S_bytes": S, "fwd_bytes": 3 * S,
               "fwd_bwd_bytes": 5 * S, **res}
        for mode, nbytes in (("fwd", 3 * S), ("fwd_bwd", 5 * S)):
            row["ours_%s_copy_frac" % mode] = nbytes / (res["ours_%s_us" % mode] * 1e-6) / COPY_RATE
        for mode, _ in modes:
            if "eager_%s_us" % mode in res:
                row["speedup_%s" % mode] = res["eager_%s_us" % mode] / res["ours_%s_us" % mode]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del leaves, w, dr
        torch.cuda.empty_cache()
    out = {"tool": "tools/bench_interpolate.py", "warmup": a.warmup, "reps": a.reps, "copy_rate_Bps": COPY_RATE,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"interpolate": [(r["shape"], round(r.get("speedup_fwd", 0), 2), round(r.get("speedup_fwd_bwd", 0), 2),
                                       round(r.get("speedup_situ", 0), 3)) for r in rows]}))


if __name__ == "__main__":
    main()
