#!/usr/bin/env python3
"""Time DiffRender.render_indexed (every image picks its mesh, texture, lights and bg row; one pass, nothing gathered) against the only routes
to the same images without it.  HIP events around `--inner` calls, warm-up first, then `--reps` timed runs of every contender in turn
(alternating: drift hits all alike); median and min-max.  Not called by bench.py.

    python tools/bench_render_indexed.py --out profiles/render_indexed_bench.json --note profiles/render_indexed_kernels.md

(a) the rainbow sheet (show_rainbow2.py:376-399): 7 meshes x 7 textures x 36 azimuths = 1764 images, forward only (no_grad), at the Market shape
    (128x64) and at 128x128
    indexed    one render_indexed over the 7 + 7 resident rows, device indices
    loop       the reference's loop: per azimuth and texture, textures[i].unsqueeze(0).repeat(7,1,1,1) and a render of the 7 shapes -- 252 calls
               (WITHOUT the reference's .cpu() per call: the loop at its best)
    gathered   index_select of vertices, textures and lights to 1764 rows (timed), then ONE render
(b) a training-shaped case at config 2 (128x128, texture 256x128): M = 96 images over 48 rows of every tensor, random indices, forward + backward,
    loss = sum(w * rgbs), gradients into the 48-row leaves
    indexed    render_indexed
    gathered   index_select of the four tensors + render + autograd's index_select backward
The bar, per shape: the indexed call's SLOWEST run is under the yardstick's FASTEST run (for (a): of the faster of the two yardsticks).
Also recorded: the index-sum kernel (its launches' durations from torch.profiler's device trace) against a device-to-device copy of the same
bytes -- the sum reads M and writes R rows, a copy reads and writes its size once: (M + R) / 2 rows --, the plan kernel's duration at M = 1764,
and, where hipcc is at hand, the compiler's resource report of the two kernels (scratch must be 0).  With --parent-lib the parent commit's library
is compared with this build's kernel by kernel (tools/kernel_disasm_diff.py) and the counts are recorded; with --earlier an earlier build's record
of this tool supplies the plan kernel's former times for the note."""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEMPLATE = "smpl_uv_642"
SHARED = ("vertices", "textures", "lights", "bg")
CAMERAS = ("azimuths", "elevations", "distances", "biases")


def stats(us):
    return {"median_us": float(np.median(us)), "min_us": float(np.min(us)), "max_us": float(np.max(us)), "runs": len(us)}


def timed(fn, ev, inner):
    ev[0].record()
    for _ in range(inner):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / inner          # us per call


def contest(contenders, ev, warmup, reps, inner, before=None):
    for _ in range(warmup):
        for _, f in contenders:
            f()
    torch.cuda.synchronize()
    times = {k: [] for k, _ in contenders}
    for _ in range(reps):
        for k, f in contenders:
            if before:
                before()
            times[k].append(timed(f, ev, inner))
    return {k: stats(v) for k, v in times.items()}


def kernel_us(fn, n_calls, names):
    """({name: durations of the launches whose kernel name holds `name`, inside n_calls runs of fn, from torch.profiler's device trace}, why not)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(n_calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for name in names:
            durs = [float(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total) for e in prof.events() if name in e.name]
            out[name] = [d for d in durs if d > 0]
        missing = [n for n in names if not out[n]]
        return out, ("torch.profiler's trace holds no launch with a device time of: " + ", ".join(missing) if missing else None)
    except Exception as e:                                   # a measurement tool: record it in the result, measure the rest
        return {n: [] for n in names}, "torch.profiler failed: %s: %s" % (type(e).__name__, e)


def kernel_resources():
    """the compiler's resource report of csrc/mm_indexed.hip for gfx950 (no GPU needed), or why there is none"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "3d-magic-mirror_amd", "csrc", "mm_indexed.hip")
    if not os.path.exists(hipcc):
        return {"unavailable": "no hipcc at " + hipcc}
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage",
           "-c", src, "-o", os.devnull]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        return {"unavailable": "hipcc failed: " + p.stderr[-400:]}
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = "index_plan_kernel" if "index_plan" in m.group(1) else ("index_sum_kernel" if "index_sum" in m.group(1) else None)
            if cur:
                out[cur] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur:
                out[cur][key] = int(m.group(1))
    out["command"] = "hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Rpass-analysis=kernel-resource-usage -c csrc/mm_indexed.hip"
    return out


def disasm_diff(parent_lib):
    """tools/kernel_disasm_diff.py of the parent commit's library against this build's, summarised"""
    new_lib = os.path.join(ROOT, "3d-magic-mirror_amd", "lib", "libmm_render.so")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kernel_disasm_diff.py"), parent_lib, new_lib, "--drop-last-false"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode not in (0, 1) or "identical machine code" not in p.stdout:
        return {"unavailable": "kernel_disasm_diff.py failed: " + (p.stderr or p.stdout)[-300:]}
    count = lambda head: int(re.search(head + r": (\d+)", p.stdout).group(1))
    return {"command": "tools/kernel_disasm_diff.py PARENT/libmm_render.so lib/libmm_render.so --drop-last-false", "exit_status": p.returncode,
            "identical": count("identical machine code"), "different": count("different machine code"), "only_old": count("only in OLD"),
            "different_names": re.findall(r"^  ! (.*?)  \(", p.stdout, re.M), "only_new": re.findall(r"^  \+ (.*?)  \(", p.stdout, re.M)}


def rainbow(pkg, dev, ev, a, S, ratio):
    """shape (a): 7 meshes x 7 textures x 36 azimuths, images in the loop's order (azimuth, texture, shape)"""
    ns, nt, na = 7, 7, 36
    dr = pkg.DiffRender(os.path.join(ROOT, "tests", "golden", "templates", TEMPLATE + ".npz"), S, ratio=ratio)
    H, W = dr.render_height, dr.image_size
    att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, ns, H, W, seed=0)
    Ae = {k: att[k].to(dev) for k in SHARED[:3] + CAMERAS}
    Ae["bg"] = None
    M = ns * nt * na
    i = torch.arange(M, device=dev)
    shape_of, tex_of, az_of = i % ns, (i // ns) % nt, i // (ns * nt)
    sheet = dict(Ae)
    for c in CAMERAS:
        sheet[c] = Ae[c][shape_of].contiguous()
    sheet["azimuths"] = (az_of.float() * 10.0).contiguous()
    index = {"vertices": shape_of, "lights": shape_of, "textures": tex_of}
    az_list = [torch.full((ns,), 10.0 * k, device=dev) for k in range(na)]

    def f_indexed():
        dr.render_indexed(index=index, **sheet)

    def f_loop():
        A_tmp = dict(Ae)
        for k in range(na):
            A_tmp["azimuths"] = az_list[k]
            for t in range(nt):
                A_tmp["textures"] = Ae["textures"][t].unsqueeze(0).repeat(ns, 1, 1, 1)
                dr.render(**A_tmp)

    def f_gathered():
        g = dict(sheet)
        g["vertices"] = Ae["vertices"].index_select(0, shape_of)
        g["lights"] = Ae["lights"].index_select(0, shape_of)
        g["textures"] = Ae["textures"].index_select(0, tex_of)
        dr.render(**g)

    with torch.no_grad():
        # the same images: the indexed sheet against the gathered render, bit for bit, before anything is timed
        r0, _ = dr.render_indexed(index=index, **sheet)
        g = dict(sheet)
        g.update(vertices=Ae["vertices"].index_select(0, shape_of), lights=Ae["lights"].index_select(0, shape_of), textures=Ae["textures"].index_select(0, tex_of))
        r1, _ = dr.render(**g)
        same = bool(torch.equal(r0, r1))
        covered = float((dr.last_face_idx >= 0).float().mean())
        del r0, r1, g
        res = contest([("indexed", f_indexed), ("loop", f_loop), ("gathered", f_gathered)], ev, a.warmup, a.reps, a.inner)
        durs, why_not = kernel_us(f_indexed, 6, ["index_plan_kernel"])
    best = min(res["loop"]["min_us"], res["gathered"]["min_us"])
    row = {"shape": "rainbow %dx%d" % (H, W), "images": M, "rows": {"vertices": ns, "textures": nt, "lights": ns}, "bit_identical_to_gathered": same,
           "covered": covered, **{k + "_" + s: x for k, d in res.items() for s, x in d.items()},
           "indexed_over_loop": res["indexed"]["median_us"] / res["loop"]["median_us"],
           "indexed_over_gathered": res["indexed"]["median_us"] / res["gathered"]["median_us"],
           "gathered_bytes": int(M * (Ae["vertices"][0].numel() + Ae["textures"][0].numel() + 9) * 4),
           "launches": {"indexed": "1 call: plan + vertex + order + raster", "loop": "%d calls" % (na * nt), "gathered": "3 index_select + 1 call"},
           "faster_beyond_spread": bool(res["indexed"]["max_us"] < best)}
    if durs["index_plan_kernel"]:
        row.update({"plan_kernel_" + s: x for s, x in stats(durs["index_plan_kernel"]).items()})
    else:
        row["plan_kernel_unmeasured"] = why_not
    print(json.dumps(row), flush=True)
    return row


def training(pkg, dev, ev, a):
    """shape (b): M = 96 images over 48 rows of every tensor at config 2, forward + backward"""
    S, R, M = 128, 48, 96
    dr = pkg.DiffRender(os.path.join(ROOT, "tests", "golden", "templates", TEMPLATE + ".npz"), S)
    att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, M, S, S, seed=0)
    g = torch.Generator().manual_seed(1)
    index = {k: torch.randint(0, R, (M,), generator=g).to(dev) for k in SHARED}
    leaves = {k: att[k][:R].to(dev).contiguous().requires_grad_(True) for k in SHARED}
    cams = {c: att[c].to(dev) for c in CAMERAS}
    w = torch.randn(M, 4, S, S, device=dev)

    def zero():
        for t in leaves.values():
            t.grad = None

    def f_indexed():
        rgbs, _ = dr.render_indexed(no_mask=True, index=index, **leaves, **cams)
        (rgbs * w).sum().backward()

    def f_gathered():
        gat = {k: leaves[k].index_select(0, index[k]) for k in SHARED}
        rgbs, _ = dr.render(no_mask=True, **gat, **cams)
        (rgbs * w).sum().backward()

    res = contest([("indexed", f_indexed), ("gathered", f_gathered)], ev, a.warmup, a.reps, a.inner, before=zero)
    shared_row_bytes = sum(leaves[k][0].numel() * 4 for k in SHARED)
    row = {"shape": "config 2, M = 96 over 48 rows", "images": M, "rows": R, **{k + "_" + s: x for k, d in res.items() for s, x in d.items()},
           "indexed_over_gathered": res["indexed"]["median_us"] / res["gathered"]["median_us"],
           "gathered_bytes": int(M * shared_row_bytes), "faster_beyond_spread": bool(res["indexed"]["max_us"] < res["gathered"]["min_us"])}
    # ---- the index-sum kernel alone, against a copy of the same bytes
    zero(); f_indexed(); zero(); f_indexed()
    durs, why_not = kernel_us(lambda: (zero(), f_indexed()), 12, ["index_sum_kernel", "index_plan_kernel"])
    nfloat = (M + R) * shared_row_bytes // 8                  # (M + R) / 2 rows, as floats
    src, dst = torch.empty(nfloat, device=dev), torch.empty(nfloat, device=dev)
    copy = contest([("copy", lambda: dst.copy_(src))], ev, a.warmup, max(a.reps, 15), 5)["copy"]
    vs = {"bytes_moved": (M + R) * shared_row_bytes, "copy_bytes": nfloat * 4, **{"copy_" + s: x for s, x in copy.items()},
          "copy_TBps": 2 * nfloat * 4 / (copy["median_us"] * 1e-6) / 1e12}
    if durs["index_sum_kernel"]:
        vs.update({"index_sum_" + s: x for s, x in stats(durs["index_sum_kernel"]).items()})
        vs["copy_frac"] = copy["median_us"] / vs["index_sum_median_us"]
        vs["index_sum_TBps"] = (M + R) * shared_row_bytes / (vs["index_sum_median_us"] * 1e-6) / 1e12
    else:
        vs["index_sum_unmeasured"] = why_not
    if durs["index_plan_kernel"]:
        vs.update({"plan_kernel_" + s: x for s, x in stats(durs["index_plan_kernel"]).items()})
    row["index_sum"] = vs
    print(json.dumps(row), flush=True)
    return row


def write_note(path, out):
    L = ["# render_indexed: the two new kernels, measured", "",
         "Written by `tools/bench_render_indexed.py` (%s; %d runs per contender, alternating, %d calls per run; figures in us)." % (
             out["device"], out["reps"], out["inner"]), ""]
    L += ["## Against the yardsticks", "", "| shape | indexed (min / median / max) | yardstick (fastest run) | indexed slowest < yardstick fastest |", "|---|---|---|---|"]
    for r in out["rainbow"]:
        L.append("| %s, %d images, forward | %.0f / %.0f / %.0f | loop of 252 calls %.0f; gathered + one render %.0f | %s |" % (
            r["shape"], r["images"], r["indexed_min_us"], r["indexed_median_us"], r["indexed_max_us"], r["loop_min_us"], r["gathered_min_us"],
            "yes" if r["faster_beyond_spread"] else "NO"))
    t = out["training"]
    L.append("| %s, forward + backward | %.0f / %.0f / %.0f | index_select + render + autograd %.0f | %s |" % (
        t["shape"], t["indexed_min_us"], t["indexed_median_us"], t["indexed_max_us"], t["gathered_min_us"], "yes" if t["faster_beyond_spread"] else "NO"))
    s = t["index_sum"]
    L += ["", "## The index sum", ""]
    if "index_sum_median_us" in s:
        L.append("M = 96 staged rows of all four tensors into 48 rows: %.1f us median (%.1f - %.1f) for %.1f MB over the bus = %.2f TB/s; a device-to-device copy "
                 "of the same bytes takes %.1f us: the kernel runs at %.2f of the copy's rate (the measure csrc/mm_views.hip quotes for its sum)." % (
                     s["index_sum_median_us"], s["index_sum_min_us"], s["index_sum_max_us"], s["bytes_moved"] / 1e6, s["index_sum_TBps"], s["copy_median_us"], s["copy_frac"]))
    else:
        L.append("Not measured: %s." % s.get("index_sum_unmeasured"))
    L += ["", "## The plan kernel", ""]
    for r in out["rainbow"]:
        if "plan_kernel_median_us" in r:
            L.append("M = %d (%s): %.1f us median (%.1f - %.1f), one workgroup per tensor, 7 chunks of 256 images." % (
                r["images"], r["shape"], r["plan_kernel_median_us"], r["plan_kernel_min_us"], r["plan_kernel_max_us"]))
        else:
            L.append("M = %d (%s): not measured: %s." % (r["images"], r["shape"], r.get("plan_kernel_unmeasured")))
    if "plan_kernel_median_us" in s:
        L.append("M = 96 over 48 rows: %.1f us median." % s["plan_kernel_median_us"])
    L += ["", "## Cross-compilation", ""]
    res = out["kernel_resources"]
    if "unavailable" in res:
        L.append("No resource report in this run: %s." % res["unavailable"])
    else:
        L.append("`%s` succeeds on a machine without a GPU (so do the touched files: the library is built the same way).  The compiler's report:" % res["command"])
        L.append("")
        for k in ("index_plan_kernel", "index_sum_kernel"):
            if k in res:
                L.append("- `%s`: %d VGPRs, %d SGPRs, scratch %d bytes per lane, %d waves per SIMD, %d bytes of LDS." % (
                    k, res[k].get("vgprs", -1), res[k].get("sgprs", -1), res[k].get("scratch_bytes_per_lane", -1), res[k].get("waves_per_simd", -1), res[k].get("lds_bytes", -1)))
    L += ["", "## The kernels of the parent build", ""]
    dd = out.get("disasm_diff")
    if not dd:
        L.append("Not compared in this run (`--parent-lib` not given).")
    elif "unavailable" in dd:
        L.append("Not compared in this run: %s." % dd["unavailable"])
    else:
        L.append("`%s` (the parent commit's library against this build's, kernel by kernel, instruction text hashed): %d kernels of the parent with identical "
                 "machine code, %d with different machine code, %d only in the parent, %d only in this build; exit status %d." % (
                     dd["command"], dd["identical"], dd["different"], dd["only_old"], len(dd["only_new"]), dd["exit_status"]))
        if dd["different_names"]:
            L += ["", "Different:"] + ["- `%s`" % n for n in dd["different_names"]]
        L += ["", "Only in this build:"] + ["- `%s`" % n for n in dd["only_new"]]
        if dd["different"] == 0 and dd["only_old"] == 0:
            L += ["", "So every kernel `mm_render_forward`, `mm_render_backward` and `mm_render_views_*` launch is the parent's, instruction for instruction (the "
                  "indexed instantiations carry one more, trailing, template argument), and `render_views` was not re-measured."]
    e = out.get("earlier")
    if e:
        L += ["", "## The plan's counters: workspace against LDS", "",
              "`%s` is the same tool's record of an earlier build of this change, whose plan kernel kept the rows' counters and fill cursors in the workspace for every "
              "row count (integer atomics in memory; this build does that above %d rows only and uses LDS words below).  The plan kernel then, and now:" % (e["file"], 8192), ""]
        now = {r["shape"]: r for r in out["rainbow"]}
        for r in e["rainbow"]:
            n = now.get(r["shape"], {})
            if "plan_kernel_median_us" in r:
                L.append("- M = %d over 7 rows (%s): %.1f us then, %s now." % (r["images"], r["shape"], r["plan_kernel_median_us"],
                                                                           ("%.1f us" % n["plan_kernel_median_us"]) if "plan_kernel_median_us" in n else "unmeasured"))
        if "plan_kernel_median_us" in e["training"]["index_sum"]:
            L.append("- M = 96 over 48 rows: %.1f us then, %s now." % (e["training"]["index_sum"]["plan_kernel_median_us"],
                     ("%.1f us" % s["plan_kernel_median_us"]) if "plan_kernel_median_us" in s else "unmeasured"))
        L += ["", "(1764 images that count into 7 rows were 1764 atomics on one cache line then.)  The indexed call as a whole at the Market shape was %.0f us (slowest run %.0f) "
              "against the gathered yardstick's fastest %.0f then." % (e["rainbow"][0]["indexed_median_us"], e["rainbow"][0]["indexed_max_us"], e["rainbow"][0]["gathered_min_us"])]
    L.append("")
    with open(path, "w") as f:
        f.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2, help="calls between the two events of one timed run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--note", default=None, help="write the short kernels note (markdown) here")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libmm_render.so: tools/kernel_disasm_diff.py is run against this build's and recorded")
    ap.add_argument("--earlier", default=None, help="this tool's --out of an earlier build (plan counters in the workspace): its plan-kernel times go into the note")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    pkg = importlib.import_module("3d-magic-mirror_amd")
    dev = torch.device("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {"tool": "tools/bench_render_indexed.py", "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "inner": a.inner,
           "rainbow": [rainbow(pkg, dev, ev, a, 64, 2), rainbow(pkg, dev, ev, a, 128, 1)]}
    torch.cuda.empty_cache()
    out["training"] = training(pkg, dev, ev, a)
    out["kernel_resources"] = kernel_resources()
    if a.parent_lib:
        out["disasm_diff"] = disasm_diff(a.parent_lib)
    if a.earlier:
        with open(a.earlier) as f:
            e = json.load(f)
        out["earlier"] = {"file": "profiles/" + os.path.basename(a.earlier), "rainbow": e["rainbow"], "training": e["training"]}
    ok = all(r["faster_beyond_spread"] and r["bit_identical_to_gathered"] for r in out["rainbow"]) and out["training"]["faster_beyond_spread"]
    out["indexed_faster_than_every_yardstick_beyond_spread"] = ok
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if a.note:
        write_note(a.note, out)
    print(json.dumps({"rainbow": [(r["shape"], round(r["indexed_over_loop"], 3), round(r["indexed_over_gathered"], 3)) for r in out["rainbow"]],
                      "training_indexed_over_gathered": round(out["training"]["indexed_over_gathered"], 3), "ok": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
