"""Step mode of the fused render + loss step (MMRenderDesc.step_grads): the backward's pixel pass runs in the forward's shade epilogue and
mm_render_backward launches only the gathers and the vertex backward.  Every test compares a RenderLossStep in step mode with the same step
with the field unset -- the standalone pixel_bwd launch -- through the C ABI, BIT FOR BIT (int32 views: signed zeros and NaN payloads count):
the image, face_idx, normals, the loss and all eight gradients.  The two paths share the pixel pass's text (csrc/mm_pixel_pass.h), the gather
re-forms dL/dalpha and its fixed-point scale exactly, and every sum is an integer sum or a fixed-order one, so nothing is "close": it is equal."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import TEMPLATES

pytestmark = pytest.mark.gpu

LEAVES = ("vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases")


def _step(pkg, name, B, S, ratio=1, seed=0, no_mask=True, step_mode=True, tex=None, loss_scale=None, contour=0.0, options=0, dist=None,
          soft_gt=False, uv_corner=False):
    """A fused RenderLossStep on seeded inputs.  tex: (Ht, Wt) of a random texture instead of the default (2H, W); dist: all cameras at this
    distance; soft_gt: a ground-truth mask with values all over [0, 1] (the default one is binary); uv_corner: every face's uvs on the corner
    shared by four texture tiles, four records per covered pixel (the record pool of the minimum workspace overflows)."""
    stepmod = importlib.import_module("3d-magic-mirror_amd.step")
    dev = torch.device("cuda:0")
    dr = pkg.DiffRender(os.path.join(TEMPLATES, name + ".npz"), S, ratio=ratio, emit_imnormal=True)
    dr.options = options
    H, W = dr.render_height, dr.image_size
    att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, B, H, W, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    if tex is not None:
        att["textures"] = torch.rand(B, 3, tex[0], tex[1], generator=g)
    if dist is not None:
        att["distances"] = torch.full((B,), float(dist)) if np.isscalar(dist) else torch.tensor(dist, dtype=torch.float32)
    if soft_gt:
        gt = gt.clone()
        gt[:, 3] = torch.rand(B, H, W, generator=g)
    if uv_corner:
        Ht, Wt = att["textures"].shape[2:]
        dr.face_uvs = torch.empty_like(dr.face_uvs)
        dr.face_uvs[..., 0] = 32.0 / Wt                           # texel coordinates (31.5, 31.5)
        dr.face_uvs[..., 1] = 1.0 - 32.0 / Ht
    att = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in att.items()}
    st = stepmod.RenderLossStep(dr, att, gt.to(dev), no_mask=no_mask, contour=contour, emit_imnormal=True, loss_scale=loss_scale, fused=True,
                                step_mode=step_mode)
    return st


def _arrays(st):
    torch.cuda.synchronize()
    out = {"rgba": st.rgba, "face_idx": st.face_idx, "face_normals": st.face_normals, "imnormal": st.imnormal, "loss": st.loss}
    out.update({"grad_" + k: v for k, v in st.grads.items() if v is not None})
    return {k: v.detach().clone() for k, v in out.items()}


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), "%s differs (max |delta| %g)" % (k, float((a[k].float() - b[k].float()).abs().nan_to_num(1e30).max()))


def _pair(pkg, *args, taken=True, **kw):
    """(step mode, field unset) of the same case, both run once"""
    new = _step(pkg, *args, step_mode=True, **kw)
    old = _step(pkg, *args, step_mode=False, **kw)
    assert new.step_mode_taken() == taken and not old.step_mode_taken()
    new.run(); old.run()
    return new, old


def _tile_counts(st):
    """(B,4) int32 of the tile order: [:, 0] tiles walked by four waves together (>= 192 candidates), [:, 1] tiles with any candidate"""
    N = importlib.import_module("3d-magic-mirror_amd._native")
    out = (ctypes.c_size_t * 4)()
    assert N.lib().mm_debug_step_layout(ctypes.byref(st.d), out) == 0
    torch.cuda.synchronize()
    return st.ws[out[0]:out[0] + st.B * 16].view(torch.int32).reshape(st.B, 4).cpu().numpy()


@pytest.mark.parametrize("S,ratio,tex", [(40, 0.6, (40, 24)), (32, 1, (64, 32)), (40, 0.6, (38, 27))])
@pytest.mark.parametrize("no_mask", [True, False])
def test_partial_blocks_tiles_and_tail_images(pkg, S, ratio, tex, no_mask):
    """24x40: a partial 16x16 block and lanes outside the image; B = 3: the tail branch of map_block; textures with a partial 32-texel tile,
    with two tiles whose border footprints straddle, and with a width that is no multiple of 4; a ground-truth mask that is not binary (the
    gather's dL/dalpha and its scale come from the mask's extremes)."""
    new, old = _pair(pkg, "sphere", 3, S, ratio=ratio, seed=21, no_mask=no_mask, tex=tex, soft_gt=True)
    assert (new.H, new.W) == ((24, 40) if S == 40 else (32, 32))
    a = _arrays(new)
    _same(a, _arrays(old))
    assert float(a["grad_textures"].abs().max()) > 0 and float(a["grad_vertices"].abs().max()) > 0
    assert (a["face_idx"] >= 0).any() and (a["face_idx"] < 0).any()


def test_close_up_takes_the_cooperative_walks_epilogue(pkg):
    new, old = _pair(pkg, "smpl_uv_642", 2, 32, seed=5, dist=[2.0, 2.6])
    cnt = _tile_counts(new)
    print("close-up tile counts {cooperative, non-empty}:", cnt[:, :2].tolist())
    assert cnt[:, 0].min() >= 1 and (cnt[:, 1] * 2 >= 16).all()   # (and at least half of the tiles have candidates)
    assert cnt[:, 0].max() >= 1                      # some tile has >= 192 candidates: only wave 0 of its workgroup shades it
    _same(_arrays(new), _arrays(old))


def test_far_camera_most_tiles_empty(pkg):
    new, old = _pair(pkg, "smpl_uv_642", 2, 32, seed=6, dist=9.0)
    cnt = _tile_counts(new)
    print("far-camera tile counts {cooperative, non-empty}:", cnt[:, :2].tolist())
    assert (cnt[:, 1] > 0).all() and (cnt[:, 1] * 2 < 16).all()     # fewer than half of an image's 16 tiles have a candidate
    _same(_arrays(new), _arrays(old))


def test_loss_scale(pkg):
    new, old = _pair(pkg, "sphere", 3, 32, seed=8, loss_scale=0.375)
    a = _arrays(new)
    _same(a, _arrays(old))
    one = _step(pkg, "sphere", 3, 32, seed=8)
    one.run()
    assert not torch.equal(_arrays(one)["grad_vertices"], a["grad_vertices"])


def test_set_inputs_rotation_over_two_batches(pkg):
    (new, old), (new2, old2) = [_pair(pkg, "sphere", 3, 32, seed=s) for s in (31, 32)]
    first, second = _arrays(new), _arrays(new2)
    own = (dict(new.inp), new.gt)
    for st in (new, old):
        st.set_inputs(new2.inp, new2.gt)
        st.run()
    a = _arrays(new)
    _same(a, _arrays(old))
    _same(a, second)                                                 # the other batch's results, on this step's buffers
    new.set_inputs(*own)
    new.run()
    _same(_arrays(new), first)                                       # and back


def test_backward_twice_after_one_forward(pkg):
    new, old = _pair(pkg, "sphere", 3, 32, seed=9)
    ref = _arrays(old)
    new.run_forward(); new.run_backward()
    once = _arrays(new)
    new.run_backward()
    twice = _arrays(new)
    _same(once, twice)
    _same(once, ref)                                                 # (run_forward + run_backward is run())


def test_capture_and_replay(pkg):
    new, old = _pair(pkg, "sphere", 3, 32, seed=10)
    ref = _arrays(old)
    new.capture()
    for v in new.grads.values():
        if v is not None:
            v.zero_()
    new.replay()
    _same(_arrays(new), ref)


def test_record_pool_overflow_is_loud_as_on_the_old_path(pkg):
    """Four records per covered pixel at 32x32 against room for 9/8 per pixel: images that run out report their dropped records and get NaN
    texture gradients in every texel; the others stay finite; every other array is what the old path gives."""
    kw = dict(seed=12, dist=[1.9, 1.9, 6.5], uv_corner=True, tex=(64, 64))   # (2 x 2 texture tiles: the corner all four share)
    new, old = _pair(pkg, "sphere", 3, 32, **kw)
    a, b = _arrays(new), _arrays(old)
    dn, do = new.dropped_records(), old.dropped_records()
    print("dropped records per image, step mode / old path:", dn, do)
    assert dn[0] > 0 and dn[1] > 0 and dn[2] == 0
    assert [x > 0 for x in dn] == [x > 0 for x in do]
    gt_new, gt_old = a.pop("grad_textures"), b.pop("grad_textures")
    for i, n in enumerate(dn):
        assert bool(torch.isnan(gt_new[i]).all()) == (n > 0) and bool(torch.isfinite(gt_new[i]).all()) == (n == 0)
        assert torch.equal(torch.isnan(gt_new[i]), torch.isnan(gt_old[i]))
    assert torch.equal(_bits(gt_new[2]), _bits(gt_old[2]))
    _same(a, b)


def test_refusals_take_the_old_path(pkg):
    N = importlib.import_module("3d-magic-mirror_amd._native")
    # the contour term: RenderLossStep does not set the field ...
    c_new, c_old = _pair(pkg, "sphere", 3, 32, seed=13, contour=0.5, taken=False)
    assert not c_new.step_mode
    _same(_arrays(c_new), _arrays(c_old))
    # ... and the library ignores it if a caller sets it all the same
    c_new.d.step_grads = ctypes.addressof(c_new.g)
    assert not c_new.step_mode_taken()
    # several calls in flight: the one-tile-per-workgroup walk
    m_new, m_old = _pair(pkg, "sphere", 3, 32, seed=13, options=N.OPT_MANY_IN_FLIGHT, taken=False)
    assert m_new.step_mode
    _same(_arrays(m_new), _arrays(m_old))
    # a desc with fused_totals (deferred fusion) is never a step-mode call
    st = _step(pkg, "sphere", 3, 32, seed=13)
    assert st.step_mode_taken()
    d = st.render_desc()
    d.fused_totals = N.ptr(torch.zeros(3, 4, device=st.dev))
    assert not N.lib().mm_render_step_mode(ctypes.byref(d))
    stepmod = importlib.import_module("3d-magic-mirror_amd.step")
    for flag in (False, True):                                      # the deferred step with and without the field in its descriptors
        un = stepmod.RenderLossStep(st.dr, st.inp, st.gt, no_mask=True, emit_imnormal=True, fused=False)
        if flag:
            un.d.step_grads = ctypes.addressof(un.g)
            un.ws = torch.empty(st.dr.workspace_bytes(un.d), device=st.dev, dtype=torch.uint8)
            un.d.workspace, un.d.workspace_bytes = N.ptr(un.ws), un.ws.numel()
        un.run_deferred()
        got = _arrays(un)
        if flag:
            _same(got, ref)
        ref = got


def test_profiling_keeps_a_readable_pixel_slot(pkg):
    st = _step(pkg, "sphere", 3, 32, seed=14)
    st.enable_profiling()
    st.run()
    torch.cuda.synchronize()
    t = st.kernel_times_ms()
    assert all(np.isfinite(t[k]) and t[k] >= 0 for k in ("raster_fwd", "pixel_bwd", "gather_bwd", "vertex_bwd"))
    assert t["pixel_bwd"] < t["gather_bwd"]                         # an empty bracket
