#!/usr/bin/env python3
"""Time the MI355X FID pieces (fid.py over csrc/mm_fid.hip) against what a user has without them, by the wall clock until the result is
usable: warm-up first, then --runs alternating runs of --reps calls each, the median and the range of each form.  Not called by bench.py.

    python tools/bench_fid.py --out profiles/fid_bench.json --md profiles/fid_kernels.md
    rocprofv3 --kernel-trace -d <dir> -- python tools/bench_fid.py --only ours --runs 1 --reps 3      # kernel times, a run of their own
    python tools/bench_fid.py ... --trace <dir>                                                        # adds them to the .md

inception_input   B = 64 frames at 128 x 128 and 128 x 64 -> (64,3,299,299), synchronised.  "eager": the same composition in eager torch on
                  the device (permute, float, / 255, F.interpolate, 2 x - 1).
statistics        D = 2048, N = 4096 and N = 12936 float32 features in device memory -> float64 (mu, sigma) in device memory, synchronised.
                  "host": the reference's route, the features copied to the host, np.mean and np.cov of the float64 array on the BLAS's
                  threads (the result stays on the host, where the reference uses it); "torch_cov": torch.cov and mean in float64 on the device.
frechet_distance  D = 2048 from the N = 4096 statistics and a second set.  "ours" runs where the statistics live (the device); "sqrtm": the
                  reference's scipy.linalg.sqrtm route on the host, from host arrays.
The slow yardsticks ("host", "sqrtm", and our frechet_distance) run --slow-reps calls per run.  "bar" says whether ours' slowest run is under
the yardstick's fastest; no ratio is fixed in advance, and beating torch_cov is not a condition: what the hand-written Gram kernel buys over
rocBLAS is half the work, no N x D float64 copies, exact symmetry and a fixed order."""
import argparse
import csv
import glob
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e6          # us


def measure(impls, warmup, runs, reps):
    """impls: [(name, fn, slow)]; reps: (reps, slow_reps)"""
    for _ in range(warmup):
        for _, f, slow in impls:
            if not slow:
                f()
    for _, f, slow in impls:
        if slow:
            f()
    times = {k: [] for k, _, _ in impls}
    for _ in range(runs):                            # alternating: drift hits all alike
        for k, f, slow in impls:
            times[k].append(float(np.mean([wall(f) for _ in range(reps[1] if slow else reps[0])])))
    row = {}
    for k, t in times.items():
        row["%s_us" % k] = float(np.median(t))
        row["%s_min_us" % k], row["%s_max_us" % k], row["%s_runs_us" % k] = float(np.min(t)), float(np.max(t)), t
    return row


def bars(row, yardsticks):
    for y in yardsticks:
        if "%s_us" % y in row:
            row["speedup_vs_%s" % y] = row["%s_us" % y] / row["ours_us"]
            row["bar_%s" % y] = bool(row["ours_max_us"] < row["%s_min_us" % y])


def kernel_table(trace_dir):
    """mean duration and calls per kernel of this file's kernels, from the kernel-trace csv of a separate rocprofv3 run"""
    acc = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"].split("(")[0]
                if "fid_" in name:
                    name = "%s, %s x %s threads" % (name.split("::")[-1].split(" ")[-1], r.get("Grid_Size_X", "?"), r.get("Grid_Size_Y", "?"))
                    acc.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(v), "mean_us": float(np.mean(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))} for k, v in sorted(acc.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5, help="alternating runs of every form")
    ap.add_argument("--reps", type=int, default=20, help="calls per run; a run's time is their mean")
    ap.add_argument("--slow-reps", type=int, default=1, help="calls per run of the forms that take seconds")
    ap.add_argument("--only", choices=["all", "ours"], default="all")
    ap.add_argument("--trace", default=None, help="directory of a separate rocprofv3 --kernel-trace run: kernel times for the .md")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    pkg = importlib.import_module("3d-magic-mirror_amd")
    dev = torch.device("cuda:0")
    reps = (a.reps, a.slow_reps)
    everything = a.only == "all"
    rows = []

    for name, B, H, W in (("config2", 64, 128, 128), ("market", 64, 128, 64)):
        frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(H + W))
        out = torch.empty((B, 3, 299, 299), device=dev)

        def ours():
            pkg.inception_input(frames, out=out)
            torch.cuda.synchronize()

        def eager():
            x = F.interpolate(frames.permute(0, 3, 1, 2).float() / 255.0, (299, 299), mode="bilinear", align_corners=False)
            x = 2 * x - 1
            torch.cuda.synchronize()
            return x

        impls = [("ours", ours, False)] + ([("eager", eager, False)] if everything else [])
        row = {"piece": "inception_input", "shape": name, "B": B, "H": H, "W": W, "size": 299}
        if everything:
            ours()
            row["max_abs_diff_vs_eager"] = float((out - eager()).abs().max())
        row.update(measure(impls, a.warmup, a.runs, reps))
        bars(row, ["eager"])
        rows.append(row)
        print(json.dumps(row), flush=True)

    D, stats = 2048, {}
    for Nrows in (4096, 12936):
        g = torch.Generator(device=dev).manual_seed(Nrows)
        x = torch.rand((Nrows, D), device=dev, generator=g) ** 2 * (0.25 + torch.rand((1, D), device=dev, generator=g))
        st = pkg.FidStatistics(D, capacity=Nrows).update(x)

        def ours():
            st.mu = st.sigma = None
            st.finalize()
            torch.cuda.synchronize()

        def host():
            act = x.cpu().numpy().astype(np.float64)
            return np.mean(act, axis=0), np.cov(act, rowvar=False)

        def torch_cov():
            xd = x.double()
            r = xd.mean(0), torch.cov(xd.T)
            torch.cuda.synchronize()
            return r

        impls = [("ours", ours, False)] + ([("host", host, True), ("torch_cov", torch_cov, False)] if everything else [])
        row = {"piece": "statistics", "N": Nrows, "D": D}
        if everything:
            ours()
            mu, sigma = st.finalize()
            hm, hs = host()
            row["max_abs_diff_vs_host"] = float(np.abs(sigma.cpu().numpy() - hs).max())
            row["max_abs_diff_vs_torch_cov"] = float((sigma - torch_cov()[1]).abs().max())
            row["sigma_symmetric"] = bool(torch.equal(sigma, sigma.T))
        row.update(measure(impls, a.warmup, a.runs, reps))
        bars(row, ["host", "torch_cov"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        if Nrows == 4096:
            ours()
            stats["a"] = st.finalize()
            y = torch.rand((Nrows, D), device=dev, generator=g) ** 3 * (0.25 + torch.rand((1, D), device=dev, generator=g))
            stats["b"] = pkg.FidStatistics(D, capacity=Nrows).update(y).finalize()

    (m1, s1), (m2, s2) = stats["a"], stats["b"]
    hm1, hs1, hm2, hs2 = (t.cpu().numpy() for t in (m1, s1, m2, s2))
    last = {}

    def ours():
        last["ours"] = pkg.frechet_distance(m1, s1, m2, s2)

    def sqrtm():
        import scipy.linalg
        covmean, _ = scipy.linalg.sqrtm(hs1.dot(hs2), disp=False)
        d = hm1 - hm2
        last["sqrtm"] = float(d.dot(d) + np.trace(hs1) + np.trace(hs2) - 2 * np.trace(covmean.real))

    impls = [("ours", ours, True)] + ([("sqrtm", sqrtm, True)] if everything else [])
    row = {"piece": "frechet_distance", "D": D, "device": str(s1.device)}
    row.update(measure(impls, 0, a.runs, reps))
    row["value"] = last["ours"]
    if everything:
        row["value_sqrtm"] = last["sqrtm"]
    bars(row, ["sqrtm"])
    rows.append(row)
    print(json.dumps(row), flush=True)

    out = {"tool": "tools/bench_fid.py", "warmup": a.warmup, "runs": a.runs, "reps": a.reps, "slow_reps": a.slow_reps,
           "device": torch.cuda.get_device_name(0), "FID_SPLIT": pkg.FID_SPLIT, "rows": rows}
    if a.trace:
        out["kernels"] = kernel_table(a.trace)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if a.md:
        lines = ["# FID pieces on the MI355X (tools/bench_fid.py)", "",
                 "%d alternating runs of %d calls (%d for the forms that take seconds); median [min, max] of the runs' means, microseconds." % (a.runs, a.reps, a.slow_reps),
                 "The last column says whether our slowest run is under that yardstick's fastest.", "", "| piece | case | form | us | bar |", "|---|---|---|---|---|"]
        for r in rows:
            case = ", ".join("%s=%s" % (k, r[k]) for k in ("shape", "N", "D") if k in r)
            for k in ("ours", "eager", "host", "torch_cov", "sqrtm"):
                if "%s_us" % k in r:
                    lines.append("| %s | %s | %s | %.1f [%.1f, %.1f] | %s |" % (r["piece"], case, k, r["%s_us" % k], r["%s_min_us" % k], r["%s_max_us" % k],
                                                                               "" if k == "ours" else ("ours under" if r["bar_%s" % k] else "ours NOT under")))
        if a.trace:
            lines += ["", "## Kernel times (a separate `rocprofv3 --kernel-trace` run of `--only ours`)", "", "| kernel | calls | mean us | min | max |", "|---|---|---|---|---|"]
            lines += ["| %s | %d | %.1f | %.1f | %.1f |" % (k, v["calls"], v["mean_us"], v["min_us"], v["max_us"]) for k, v in out["kernels"].items()]
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"fid": [(r["piece"], r.get("shape", r.get("N", r.get("D"))), {k: v for k, v in r.items() if k.startswith(("bar_", "speedup_"))}) for r in rows]}))


if __name__ == "__main__":
    main()
