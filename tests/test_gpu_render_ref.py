"""The device against autograd: the fused render's forward and every input gradient held DIRECTLY to tests/render_ref.py -- the render's forward
restated in torch float64, its derivative autograd's -- on the edge cases of tests/render_ref_cases.py, instead of to the C oracle alone,
whose backward the kernels were derived beside.  tests/test_render_ref_host.py holds the oracle to the same reference.

The reference is evaluated in float64 on the fp32 inputs with `face_idx=` the device's own map, so both differentiate the same pixels.
Bar, for rgba (absolute) and for every gradient (relative to the reference's maximum) -- parity_bar's conditioning rule as one inequality:

    e_hip <= 1e-4 + 2 * e_o32

e_o32: the fp32 ORACLE's own distance from the same reference, computed here; 1e-4: BASELINE's north star.  The second term is fp32
conditioning of the mult = 1000 edge functions (the fp32 oracle alone is up to 7e-5 from the reference in rgba and 1.5e-4 in a camera scalar:
profiles/render_ref_parity.md), not slack: e_o32 itself may not exceed 3e-4 (test_render_ref_host.py checks that without a GPU), and the
device's face_idx may differ from the reference's own float64 map in at most 0.5 % of the pixels.

Entry points: DiffRender.render under seeded noise on rgba and the face normals; render_recon and the fused step (step mode) under the loss's
own gradient; for three cases the un-fused operator chain (shim_chain.render: prepare_vertices, dibr_rasterization, texture_mapping,
spherical_harmonic_lighting), under the noise.  The coincident-corner case (a face collapsed to a point, an edge collapsed; no upstream
gradient on the collapsed faces' normals) additionally asserts finite gradients, and compares the vertex gradient with coincident vertices
summed (render_ref_cases.merge_twins says why)."""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

import render_ref_cases as C
from conftest import TEMPLATES
from parity_bar import rel_errors

pytestmark = pytest.mark.gpu
CHAIN_CASES = ("sphere_bg", "uv_border", "lights_x3")          # dibr_rasterization's default constants, the template's texture shape


def _device(pkg, case):
    """(DiffRender set up for the case, its attributes on the device as leaves, gt on the device)."""
    dev = torch.device("cuda:0")
    sp = case.spec
    dr = pkg.DiffRender(os.path.join(TEMPLATES, sp.template + ".npz"), sp.S, ratio=sp.ratio)
    assert (dr.render_height, dr.image_size) == (case.H, case.W) and np.array_equal(dr.faces.numpy(), case.inp["faces"])
    assert np.allclose(dr.cam_proj.numpy().reshape(3), case.proj, rtol=0, atol=0)
    dr.face_uvs = torch.from_numpy(case.inp["face_uvs"])[None].clone()
    dr.sigmainv, dr.boxlen, dr.knum, dr.multiplier, dr.eps = (case.kw[k] for k in ("sigmainv", "boxlen", "knum", "mult", "eps"))
    datt = {k: torch.from_numpy(case.inp[k]).to(dev).requires_grad_(True) for k in C.LEAVES if case.inp.get(k) is not None}
    datt.setdefault("bg", None)
    return dr, datt, torch.from_numpy(case.gt).to(dev)


@functools.lru_cache(maxsize=None)
def _own_map(name):
    """The reference's own float64 face map (what the device's map may leave in 0.5 % of the pixels)."""
    case = C.build(name)
    w, wfn = C.upstream_noise(case)
    return C.reference(case, w, wfn).fidx


@functools.lru_cache(maxsize=None)
def _yardstick(name, up, fidx_bytes):
    """(reference under the device's map, e_o32): built once per (case, upstream, map) and shared by the entry points."""
    case = C.build(name)
    fidx = np.frombuffer(fidx_bytes, np.int32).reshape(2, case.H, case.W)
    if up == "noise":
        w, wfn = C.upstream_noise(case)
    else:                                                          # recon_data's float64 gradient on the reference's own image
        probe = C.reference(case, np.zeros((2, case.H, case.W, 4)), None, face_idx=fidx)
        w, wfn = C.upstream_of(case, up, probe.rgba, np.float64)
    ref = C.reference(case, w, wfn, face_idx=fidx)
    o32 = C.oracle_run(case, up, np.float32)
    e = {"rgba": float(np.abs(o32.rgba.astype(np.float64) - ref.rgba).max()), "face_normals": float(np.abs(o32.fn.astype(np.float64) - ref.fn).max()),
         "imnormal": float(np.abs(o32.imn.astype(np.float64) - ref.imn).max())}
    for k in C.leaves(case):
        e[k] = rel_errors(_merged(case, k, o32.grads[k]), _merged(case, k, ref.grads[k]))[0]
    return ref, e


def _merged(case, k, g):
    g = np.asarray(g.detach().cpu().numpy() if torch.is_tensor(g) else g, np.float64)
    return C.merge_twins(case, g) if (k == "vertices" and case.twins) else g


def _hold(name, up, what, rgba, fidx, grads, fn=None, imn=None):
    """rgba (B,H,W,4), fidx (B,H,W), grads {leaf: tensor}, face normals and imnormal where the entry point returns them: the device's, against
    the bar of the module docstring (the two normal outputs: absolute, like rgba)."""
    case = C.build(name)
    fidx = np.ascontiguousarray(fidx.cpu().numpy(), dtype=np.int32)
    differ = int((fidx != _own_map(name)).sum())
    ref, e32 = _yardstick(name, up, fidx.tobytes())
    e_hip = {"rgba": float(np.abs(rgba.detach().cpu().numpy().astype(np.float64) - ref.rgba).max())}
    for k, got, want in (("face_normals", fn, ref.fn), ("imnormal", imn, ref.imn)):
        if got is not None:
            e_hip[k] = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max())
    for k in C.leaves(case):
        if case.twins:
            assert bool(torch.isfinite(grads[k]).all()), (what, k)
        e_hip[k] = rel_errors(_merged(case, k, grads[k]), _merged(case, k, ref.grads[k]))[0]
    print("%s %s %s: face_idx differs from the float64 map in %d pixels; " % (name, up, what, differ)
          + " ".join("%s e_hip=%.2e e_o32=%.2e" % (k, e_hip[k], e32[k]) for k in e_hip))
    assert differ <= 0.005 * fidx.size, (what, differ)
    assert (fidx >= 0).mean() > 0.03
    for k, e in e_hip.items():
        assert e32[k] <= 3e-4, (what, k, e32[k])
        assert e <= 1e-4 + 2 * e32[k], (what, k, e, e32[k])
    for k in C.leaves(case):
        assert float(np.abs(ref.grads[k]).max()) > 0, k


@pytest.mark.parametrize("name", C.DEVICE_CASES)
def test_render_under_noise_matches_autograd(pkg, name):
    case = C.build(name)
    dr, datt, gt = _device(pkg, case)
    w, wfn = C.upstream_noise(case)
    rgbs, out = dr.render(no_mask=case.no_mask, **datt)
    ((rgbs.permute(0, 2, 3, 1) * torch.from_numpy(w).to(gt.device)).sum() + (out["face_normals"] * torch.from_numpy(wfn).to(gt.device)).sum()).backward()
    torch.cuda.synchronize()
    _hold(name, "noise", "render", rgbs.permute(0, 2, 3, 1), dr.last_face_idx, {k: datt[k].grad for k in C.leaves(case)},
          fn=out["face_normals"], imn=out["imnormal"])


@pytest.mark.parametrize("name", C.DEVICE_CASES)
def test_render_recon_and_step_mode_under_the_loss_match_autograd(pkg, name):
    case = C.build(name)
    dr, datt, gt = _device(pkg, case)
    loss, rgbs, out = dr.render_recon(gt, no_mask=case.no_mask, **datt)
    loss.backward()
    torch.cuda.synchronize()
    _hold(name, "loss", "render_recon", rgbs.permute(0, 2, 3, 1), dr.last_face_idx, {k: datt[k].grad for k in C.leaves(case)},
          fn=out["face_normals"], imn=out["imnormal"])

    stepmod = importlib.import_module("3d-magic-mirror_amd.step")
    dr2, datt2, gt2 = _device(pkg, case)
    plain = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in datt2.items()}
    step = stepmod.RenderLossStep(dr2, plain, gt2, no_mask=case.no_mask, fused=True, step_mode=True)
    step.run()
    torch.cuda.synchronize()
    print(name, "step mode taken:", step.step_mode_taken())
    assert step.step_mode_taken() or name != "sphere_bg"
    _hold(name, "loss", "fused step", step.rgba, step.face_idx, {k: step.grads[k] for k in C.leaves(case)})


@pytest.mark.parametrize("name", CHAIN_CASES)
def test_unfused_operator_chain_under_noise_matches_autograd(pkg, name):
    chain = importlib.import_module("3d-magic-mirror_amd.shim_chain")
    case = C.build(name)
    assert all(case.kw[k] == v for k, v in C.R.DEFAULTS.items())
    dr, datt, gt = _device(pkg, case)
    w, wfn = C.upstream_noise(case)
    rgbs, fn, fidx = chain.render(dr, no_mask=case.no_mask, **datt)
    ((rgbs.permute(0, 2, 3, 1) * torch.from_numpy(w).to(gt.device)).sum() + (fn * torch.from_numpy(wfn).to(gt.device)).sum()).backward()
    torch.cuda.synchronize()
    _hold(name, "noise", "operator chain", rgbs.permute(0, 2, 3, 1), fidx.reshape(2, case.H, case.W), {k: datt[k].grad for k in C.leaves(case)}, fn=fn)
