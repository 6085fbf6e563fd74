"""The C oracle's hand-derived render_backward (oracle/mm_oracle.inc) against autograd: tests/render_ref.py restates the
render's forward in torch float64 and leaves the derivative to autograd; here the float64 oracle must agree with it ELEMENTWISE, in every
input gradient, on cases bent towards the branches that touch only a few pixels or faces (tests/render_ref_cases.py).

(a) face_idx equal; rgba, face normals and imnormal within 1e-8 absolute; each of the eight input gradients within 1e-7 of its own maximum
    (parity_bar.rel_errors, no floor) and non-zero -- under seeded noise on rgba and the face normals together, and under recon_data's own
    gradient at contour 0 and 0.3.  The two bars are 10x and 100x the worst figures of the prototype this file grew from (8.3e-10, 5.8e-10)
    and 1000x under the GPU bar; they are not measurements of the code under test.  Measured: profiles/render_ref_parity.md.
(b) each case reaches the branch it is named for (render_ref's reach counters).
(c) each deliberate wrong derivative of render_ref.FAULTS leaves the unfaulted reference, in the case built for it, by at least ten times
    the widest bar tests/test_gpu_render_ref.py applies in that case (1e-4 + 2 e_o32, e_o32 the fp32 oracle's own distance from the
    reference): a device that made that mistake would fail there.
    bary_eps_dropped is NOT in the list: the eps under the barycentrics' sum matters where the sum (twice the face's area in multiplier units,
    1e3 for a face a pixel large) is comparable to 1e-8, and a face collapsed exactly has three edge functions that cancel exactly -- it covers no
    pixel, so the term is never differentiated there.  Measured on the coincident-corner case: the fault moves no gradient by more than
    1.2e-10 of its maximum, against a bar of 2.6e-4 (test_bary_eps_cannot_be_made_visible keeps that true); it is left to the forward's comparison of rgba.
    normal_eps_dropped is judged under noise on the collapsed faces' normals too (nothing else differentiates through a zero normal), against the
    case's bar under the upstream gradients the GPU test uses.
The vertex gradient of the coincident-corner case is compared with coincident vertices summed (render_ref_cases.merge_twins), and the
close-camera case has a target mask of ones (render_ref_cases.build): both are properties of the operation, explained where they are applied.
lights x -1 is applied to image 1 alone: an image whose lights are all negated saturates at 0 in every pixel, and its texture, light and
background gradients are exactly zero -- compared as such, while image 0 keeps every gradient's maximum non-zero, as (a) requires."""
import functools
import types

import numpy as np
import pytest
import torch

import render_ref as R
import render_ref_cases as C
from parity_bar import rel_errors
from render_ref_cases import oracle_run, reference, upstream_of

UPSTREAMS = ("noise", "loss", "loss_contour")
RUNS = [(n, u) for n in C.SPECS for u in UPSTREAMS] + [("coincident", "noise_all")]
# fault -> (the case built for it, the upstream gradient it is judged under, the counters it needs)
FAULT_CASES = {
    "soft_vertex_regions_dropped": ("cut_lists", "loss", ("region_first", "region_second")),
    "soft_excl_includes_self": ("deep_lists", "loss", ("list_entries",)),
    "soft_skips_culled": ("inside_out", "loss", ("culled_entries",)),
    "clamp_passes_gradient": ("lights_x3", "noise", ("rgb_clamped_1",)),
    "border_uv_gradient_not_gated": ("uv_border", "noise", ("u_clamped_lo", "u_clamped_hi", "v_clamped_lo", "v_clamped_hi")),
    "normal_eps_dropped": ("coincident", "noise_all", ("zero_length_edges",)),
    "elevation_chain_dropped": ("steep_elevation", "noise", ()),
    "bg_weight_wrong": ("sphere_bg", "noise", ()),
}
# case -> counters that must be > 0 (what the case is named for)
REACH = {
    "sphere_bg": ("region_first", "region_interior", "region_second", "culled_entries"),
    "sphere_white": ("region_first", "region_interior", "region_second", "culled_entries"),
    "uv_seams": ("covered", "list_entries"),
    "ratio2": ("covered", "list_entries"),
    "cut_lists": ("cut_pixels", "region_first", "region_second"),
    "deep_lists": ("list_entries",),
    "uv_border": ("u_clamped_lo", "u_clamped_hi", "v_clamped_lo", "v_clamped_hi"),
    "lights_x3": ("rgb_clamped_1",),
    "lights_neg": ("rgb_clamped_0",),
    "steep_elevation": ("covered", "list_entries"),
    "close_camera": ("covered",),
    "texture_1x3": ("v_clamped_lo", "v_clamped_hi"),
    "texture_3x1": ("u_clamped_lo", "u_clamped_hi"),
    "inside_out": ("culled_entries",),
    "coincident": ("zero_length_edges",),
    "depth_tie": ("depth_ties",),
}


@functools.lru_cache(maxsize=None)
def pair(name, up):
    """The float64 oracle and the reference under the same upstream gradient (the oracle's)."""
    case = C.build(name)
    o = oracle_run(case, up, np.float64)
    return case, o, reference(case, o.w, o.wfn)


@functools.lru_cache(maxsize=None)
def e_o32(name, up):
    """The fp32 oracle's own distance from the reference: {"rgba": absolute, leaf: relative to the reference's maximum}."""
    case, _, r = pair(name, up)
    o = oracle_run(case, up, np.float32)
    out = {"rgba": float(np.abs(o.rgba.astype(np.float64) - r.rgba).max()), "fidx": int((o.fidx != r.fidx).sum())}
    if up.startswith("loss"):                     # the fp32 oracle's loss gradient is its own: the reference gets the float64 one of its own image
        w, wfn = upstream_of(case, up, r.rgba, np.float64)
        r = reference(case, w, wfn)
    out.update({k: rel_errors(o.grads[k], r.grads[k])[0] for k in C.leaves(case)})
    return out


def collapsed_vertices(case):
    m = np.zeros(case.inp["vertices"].shape[1], bool)
    m[np.unique(case.inp["faces"][case.collapsed])] = True
    return m


def figures(name, up):
    """{what: error} of the float64 oracle against the reference (forward absolute, gradients relative), for the test and the profile."""
    case, o, r = pair(name, up)
    fig = {"fidx": int((o.fidx != r.fidx).sum()), "rgba": float(np.abs(o.rgba - r.rgba).max()), "fn": float(np.abs(o.fn - r.fn).max()),
           "imn": float(np.abs(o.imn - r.imn).max())}
    if case.twins and up != "noise_all":       # (under noise_all the collapsed corners carry dn / 1e-10: the twins' split is 1e-12 of that, and their sum cancels it)
        o = types.SimpleNamespace(**dict(vars(o), grads=dict(o.grads, vertices=C.merge_twins(case, o.grads["vertices"]))))
        r = types.SimpleNamespace(**dict(vars(r), grads=dict(r.grads, vertices=C.merge_twins(case, r.grads["vertices"]))))
    for k in C.leaves(case):
        if k == "vertices" and up == "noise_all":
            # gradients through a collapsed face's normal are dn / 1e-10 large: its corners on their own maximum, the rest on theirs
            m = collapsed_vertices(case)
            fig["vertices (collapsed corners)"] = rel_errors(o.grads[k][:, m], r.grads[k][:, m])[0]
            fig["vertices (the rest)"] = rel_errors(o.grads[k][:, ~m], r.grads[k][:, ~m])[0]
            assert np.abs(r.grads[k][:, m]).max() > 1e6 * np.abs(r.grads[k][:, ~m]).max()
        else:
            fig[k] = rel_errors(o.grads[k], r.grads[k])[0]
    return fig


@pytest.mark.parametrize("name,up", RUNS)
def test_oracle_backward_is_autograd_of_the_restated_forward(name, up):
    case, o, r = pair(name, up)
    fig = figures(name, up)
    print(name, up, " ".join("%s=%.2e" % kv for kv in fig.items()))
    assert fig["fidx"] == 0
    for k in ("rgba", "fn", "imn"):
        assert fig[k] <= 1e-8, (k, fig[k])
    for k, e in fig.items():
        if k not in ("fidx", "rgba", "fn", "imn"):
            assert e <= 1e-7, (k, e)
    for k in C.leaves(case):
        assert np.isfinite(r.grads[k]).all() and np.isfinite(o.grads[k]).all(), k
        assert float(np.abs(r.grads[k]).max()) > 0 and float(np.abs(o.grads[k]).max()) > 0, k


@pytest.mark.parametrize("name", list(C.SPECS))
def test_case_reaches_its_edge(name):
    case, o, r = pair(name, "noise")
    print(name, r.cnt)
    for k in REACH[name]:
        assert r.cnt[k] > 0, (k, r.cnt)
    assert r.cnt["covered"] > 0.03 * o.fidx.size
    if name == "inside_out":
        assert r.cnt["covered"] == 0 or (r.fn[..., 2][np.arange(2)[:, None, None], np.maximum(r.fidx, 0)][r.fidx >= 0] >= 0).all()
        assert r.cnt["culled_entries"] > 0.3 * r.cnt["list_entries"]
    if name == "deep_lists":
        assert r.cnt["list_entries"] > 10 * (o.fidx < 0).sum()         # more than ten faces per uncovered pixel, on average
    if name == "lights_x3":
        assert r.cnt["rgb_clamped_1"] > 0.3 * 3 * r.cnt["covered"]
    if name == "coincident":
        assert case.collapsed.sum() >= 3 and (r.fn[:, case.collapsed] == 0).all()
        assert (np.abs(r.fn[:, ~case.collapsed]).sum(-1) > 0).all()
    if name == "depth_tie":
        assert r.cnt["depth_ties"] >= 2


@pytest.mark.parametrize("fault", list(FAULT_CASES))
def test_each_fault_is_visible_far_above_the_gpu_bar(fault):
    name, up, needs = FAULT_CASES[fault]
    case, o, r = pair(name, up)
    for k in needs:
        assert r.cnt[k] > 0, (k, r.cnt)
    f = reference(case, o.w, o.wfn, faults=(fault,))
    assert np.abs(f.rgba - r.rgba).max() <= 1e-12 and (f.fidx == r.fidx).all()         # a wrong DERIVATIVE: the forward is unchanged
    moved = {k: rel_errors(f.grads[k], r.grads[k])[0] for k in C.leaves(case)}
    e32 = e_o32(name, "noise" if up == "noise_all" else up)       # (the GPU test gives the collapsed faces' normals no upstream gradient)
    bar = max(1e-4 + 2 * e32[k] for k in C.leaves(case))
    worst = max(moved, key=moved.get)
    print(fault, name, up, "moved %s by %.3e; widest GPU bar %.3e" % (worst, moved[worst], bar))
    assert moved[worst] >= 10 * bar, (moved, bar)


def test_bary_eps_cannot_be_made_visible():
    """The docstring's claim about bary_eps_dropped, kept true: on the coincident-corner case it moves nothing measurable."""
    case, o, r = pair("coincident", "noise_all")
    f = reference(case, o.w, o.wfn, faults=("bary_eps_dropped",))
    assert max(rel_errors(f.grads[k], r.grads[k])[0] for k in C.leaves(case)) < 1e-9


@pytest.mark.parametrize("name", C.DEVICE_CASES)
def test_the_fp32_oracle_is_within_reach_of_the_reference(name):
    """The GPU test's condition on its own yardstick, checked here, before any GPU run: e_o32 <= 3e-4 in every case it uses, and the fp32
    oracle sees the faces the reference sees."""
    for up in ("noise", "loss"):
        e = e_o32(name, up)
        print(name, up, " ".join("%s=%.2e" % kv for kv in e.items()))
        assert e["fidx"] == 0
        assert max(v for k, v in e.items() if k != "fidx") <= 3e-4, e
