"""Writes profiles/render_ref_parity.md: the figures behind tests/test_render_ref_host.py (computed here, CPU only) and, from the `-s` output of
`pytest -m gpu tests/test_gpu_render_ref.py` given as arguments, the device's.

    python profiles/tools/render_ref_parity.py gpu_log [gpu_log ...] > profiles/render_ref_parity.md"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np                                                  # noqa: E402
import render_ref_cases as C                                        # noqa: E402
import test_render_ref_host as T                                    # noqa: E402
from parity_bar import rel_errors                                   # noqa: E402


def host():
    print("## 1. The float64 oracle against the reference (CPU)\n")
    print("Forward: max absolute difference.  Gradients: max|oracle - reference| / max|reference|, the worst of the eight inputs and which.")
    print("Bars: 1e-8 and 1e-7.  face_idx is equal in every run.\n")
    print("| case | upstream | rgba | face normals | imnormal | worst gradient | input |")
    print("|---|---|---|---|---|---|---|")
    worst_f, worst_g = 0.0, 0.0
    for name, up in T.RUNS:
        fig = T.figures(name, up)
        assert fig["fidx"] == 0
        g = {k: v for k, v in fig.items() if k not in ("fidx", "rgba", "fn", "imn")}
        k = max(g, key=g.get)
        worst_f, worst_g = max(worst_f, fig["rgba"], fig["fn"], fig["imn"]), max(worst_g, g[k])
        print("| %s | %s | %.1e | %.1e | %.1e | %.1e | %s |" % (name, up, fig["rgba"], fig["fn"], fig["imn"], g[k], k))
    print("\nWorst forward figure %.1e, worst gradient figure %.1e.\n" % (worst_f, worst_g))
    print("## 2. What each case reaches (render_ref's counters, both images)\n")
    keys = ("covered", "list_entries", "cut_pixels", "region_first", "region_interior", "region_second", "culled_entries", "zero_length_edges",
            "u_clamped_lo", "u_clamped_hi", "v_clamped_lo", "v_clamped_hi", "rgb_clamped_0", "rgb_clamped_1", "depth_ties")
    print("| case | " + " | ".join(keys) + " |")
    print("|---|" + "---|" * len(keys))
    for name in C.SPECS:
        cnt = T.pair(name, "noise")[2].cnt
        print("| %s | " % name + " | ".join(str(cnt[k]) for k in keys) + " |")
    print("\n## 3. Each fault's displacement beside the bar it had to beat\n")
    print("Displacement: max over the inputs of max|faulted - reference| / max|reference|.  Bar: the widest 1e-4 + 2 e_o32 of the case; the test asks 10x that.\n")
    print("| fault | case | upstream | moved | by | widest GPU bar | ratio |")
    print("|---|---|---|---|---|---|---|")
    for fault, (name, up, _) in list(T.FAULT_CASES.items()) + [("bary_eps_dropped (not in the list)", ("coincident", "noise_all", ()))]:
        case, o, r = T.pair(name, up)
        f = C.reference(case, o.w, o.wfn, faults=(fault.split()[0],))
        moved = {k: rel_errors(f.grads[k], r.grads[k])[0] for k in C.leaves(case)}
        e32 = T.e_o32(name, "noise" if up == "noise_all" else up)
        bar = max(1e-4 + 2 * e32[k] for k in C.leaves(case))
        k = max(moved, key=moved.get)
        print("| %s | %s | %s | %s | %.2e | %.2e | %.0f |" % (fault, name, up, k, moved[k], bar, moved[k] / bar))
    print("\n## 4. The fp32 oracle's own distance from the reference, e_o32 (CPU, the reference's own face map)\n")
    print("rgba absolute, gradients relative to the reference's maximum.  Condition: <= 3e-4; face_idx differences of the fp32 oracle: 0 in every case.\n")
    names = ["rgba"] + list(C.LEAVES)
    print("| case | upstream | " + " | ".join(names) + " |")
    print("|---|---|" + "---|" * len(names))
    for name in C.DEVICE_CASES:
        for up in ("noise", "loss"):
            e = T.e_o32(name, up)
            assert e["fidx"] == 0
            print("| %s | %s | " % (name, up) + " | ".join("%.1e" % e[k] if k in e else "-" for k in names) + " |")


def device(logs):
    print("\n## 5. The device against the reference (MI355X): e_hip / e_o32 per case, entry point and quantity\n")
    print("The reference takes the device's face map.  Bar: e_hip <= 1e-4 + 2 e_o32.  `differs`: pixels whose device face_idx is not the reference's own float64 one.\n")
    pat = re.compile(r"^\.?F?(\w+) (noise|loss) ([\w ]+): face_idx differs from the float64 map in (\d+) pixels; (.*)$")
    rows = []
    for path in logs:
        for line in open(path):
            m = pat.match(line.strip())
            if m:
                pairs = re.findall(r"(\w+) e_hip=(\S+) e_o32=(\S+)", m.group(5))
                rows.append((m.group(1), m.group(2), m.group(3), int(m.group(4)), pairs))
    names = ["rgba", "face_normals", "imnormal"] + list(C.LEAVES)
    print("| case | upstream | entry point | differs | " + " | ".join(names) + " |")
    print("|---|---|---|---|" + "---|" * len(names))
    worst = 0.0
    for name, up, what, differ, pairs in rows:
        d = {k: (float(a), float(b)) for k, a, b in pairs}
        worst = max([worst] + [a - 2 * b for a, b in d.values()])
        print("| %s | %s | %s | %d | " % (name, up, what, differ) + " | ".join("%.1e / %.1e" % d[k] if k in d else "-" for k in names) + " |")
    print("\n%d runs; the largest e_hip - 2 e_o32 is %.1e (bar 1e-4)." % (len(rows), worst))


if __name__ == "__main__":
    print("# The render's backward against autograd: measured figures\n")
    print("Written by profiles/tools/render_ref_parity.py.  tests/render_ref.py restates DiffRender.render in torch float64 and leaves the derivative to")
    print("autograd; tests/test_render_ref_host.py holds the C oracle to it, tests/test_gpu_render_ref.py the device.  Cases: tests/render_ref_cases.py")
    print("(B = 2; 32x32 unless named; upstream `noise`: N(0,1) on rgba and the face normals, `loss`: recon_data's gradient, `loss_contour`: at contour 0.3,")
    print("`noise_all`: the coincident case with noise on the collapsed faces' normals too).\n")
    host()
    if len(sys.argv) > 1:
        device(sys.argv[1:])
