"""The once-written outputs of the render step -- the image, the normals image, dL/dbg and dL/dtextures -- leave their kernels through the
store helpers of csrc/mm_device.h (store_once: a cache policy on the store, one wide store per lane; profiles/store_policy_ab.md says which
policy and why).  A store policy cannot change a value; what it can get wrong is
WHERE a store lands and HOW WIDE it is.  These tests pin addresses, widths and edges: screens and textures that are no multiple of a tile,
output arrays at 4-byte-aligned but otherwise odd addresses between guard words, batches that leave the four-tiles-per-wave path a partial
group, and the multi-view and indexed instantiations of the same kernel text.  Everything is compared through the C ABI as int32 views."""
import os

import numpy as np
import pytest
import torch

from conftest import TEMPLATES
from parity_bar import grad_close

import test_gpu_render_indexed as ix
import test_gpu_render_views as vw
from test_gpu_fused_step import LEAVES, _arrays, _bits, _pair, _same

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA1AB1E


def _make(pkg, B, S, ratio, seed, no_mask=True, step_mode=True, imn=True, tex=None, dist=None):
    """A fused RenderLossStep on seeded inputs of the sphere, and what the oracle needs to redo it"""
    import importlib
    stepmod = importlib.import_module("3d-magic-mirror_amd.step")
    dev = torch.device("cuda:0")
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), S, ratio=ratio, emit_imnormal=imn)
    H, W = dr.render_height, dr.image_size
    att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, B, H, W, seed=seed)
    if tex is not None:
        att["textures"] = torch.rand(B, 3, tex[0], tex[1], generator=torch.Generator().manual_seed(500 + seed))
    if dist is not None:
        att["distances"] = torch.full((B,), float(dist))
    inp = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in att.items()}
    inp["faces"] = dr.faces.numpy().astype(np.int32)
    inp["face_uvs"] = dr.face_uvs.numpy()[0]
    datt = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in att.items()}
    st = stepmod.RenderLossStep(dr, datt, gt.to(dev), no_mask=no_mask, emit_imnormal=imn, fused=True, step_mode=step_mode)
    return st, dr, inp, gt.numpy()


def _results(st):
    """_arrays of test_gpu_fused_step for a step that may have no normals image"""
    torch.cuda.synchronize()
    out = {"rgba": st.rgba, "face_idx": st.face_idx, "face_normals": st.face_normals, "loss": st.loss}
    if st.imnormal is not None:
        out["imnormal"] = st.imnormal
    out.update({"grad_" + k: v for k, v in st.grads.items() if v is not None})
    return {k: v.detach().clone() for k, v in out.items()}


@pytest.mark.parametrize("imn", [True, False], ids=["imnormal", "no imnormal"])
@pytest.mark.parametrize("no_mask", [True, False], ids=["bg", "white"])
@pytest.mark.parametrize("S,ratio,hw", [(20, 0.6, (12, 20)), (36, 7.0 / 9.0, (28, 36))], ids=["20x12", "36x28"])
def test_ragged_screens(pkg, oracle, S, ratio, hw, no_mask, imn):
    """W and H no multiples of the 8-pixel tile (partial tile rows: the 16- and 12-byte stores of lanes outside the image must not happen),
    B = 3: step mode and the standalone pixel backward give the same bits, and both are the oracle's numbers at the suite's bars."""
    res = []
    for step_mode in (True, False):
        st, dr, inp, gt = _make(pkg, 3, S, ratio, seed=41, no_mask=no_mask, step_mode=step_mode, imn=imn)
        assert (st.H, st.W) == hw and st.step_mode_taken() == step_mode
        st.run()
        res.append(_results(st))
    new, old = res
    _same(new, old)
    assert ("imnormal" in new) == imn and ("grad_bg" in new) == no_mask
    H, W = hw
    proj = dr.cam_proj.numpy().reshape(3)
    rgba_o, fidx_o, fn_o, imn_o = oracle.render_forward(inp, H, W, no_mask, proj)
    loss_o, dpred = oracle.recon_data(rgba_o.transpose(0, 3, 1, 2), gt, image_weight=dr.image_weight, want_grad=True)
    drgba = np.ascontiguousarray(dpred.transpose(0, 2, 3, 1))
    g_o = oracle.render_backward(inp, H, W, no_mask, proj, drgba, None)
    g64 = {}

    def ref64(k):
        if not g64:
            g64.update(oracle.render_backward(inp, H, W, no_mask, proj, drgba.astype(np.float64), None, dtype=np.float64))
        return g64[k]
    fidx = new["face_idx"].cpu().numpy()
    assert (fidx == fidx_o).all() and (fidx >= 0).any() and (fidx < 0).any()
    assert float(np.abs(new["rgba"].cpu().numpy() - rgba_o).max()) <= 1e-4
    assert float(np.abs(new["face_normals"].cpu().numpy() - fn_o).max()) <= 1e-6
    if imn:
        assert float(np.abs(new["imnormal"].cpu().numpy() - imn_o).max()) <= 1e-6
    assert abs(float(new["loss"]) - loss_o) < 2e-5
    for k in LEAVES:
        if k == "bg" and not no_mask:
            continue
        assert float(np.abs(g_o[k]).max()) > 0, k
        grad_close(new["grad_" + k], g_o[k], rtol=1e-4, what=k, ref64=lambda k=k: ref64(k))


def _carve(sizes, offsets, dev):
    """One sentinel-filled int32 buffer with arrays of `sizes` bytes inside, array i starting `offsets[i]` bytes behind a 256-byte boundary
    (of the ADDRESS) with at least 256 guard bytes on either side.  Returns the buffer, and per array its first word's index."""
    starts, o = [], 512
    for n, off in zip(sizes, offsets):
        o = (o + 255) // 256 * 256
        starts.append(o + off)
        o = o + off + n + 256
    buf = torch.full(((o + 1024) // 4,), SENTINEL, dtype=torch.int32, device=dev)
    shift = (-buf.data_ptr()) % 256                              # (the allocator hands out 256-byte-aligned blocks: 0)
    assert shift % 4 == 0
    return buf, [(s + shift) // 4 for s in starts]


@pytest.mark.parametrize("step_mode", [True, False], ids=["step", "pixel_bwd"])
@pytest.mark.parametrize("offsets", [(4, 12, 20, 4), (12, 20, 4, 12), (20, 4, 12, 20)], ids=lambda o: "+%d+%d+%d+%d" % o)
def test_guard_bands(pkg, step_mode, offsets):
    """rgba, imnormal, grad_bg and grad_textures carved out of one sentinel-filled buffer at 4-byte-aligned but otherwise odd addresses: a step
    leaves every guard word as it was, and every word inside is the word of the run with naturally aligned arrays.  28x36 screen (partial
    tiles), 48x40 texture (a partial 32-texel tile)."""
    kw = dict(B=3, S=36, ratio=7.0 / 9.0, seed=43, step_mode=step_mode, tex=(48, 40))
    ref, _, _, _ = _make(pkg, **kw)
    ref.run()
    want = _results(ref)
    st, _, _, _ = _make(pkg, **kw)
    names = ("rgba", "imnormal", "grad_bg", "grad_textures")
    like = (st.rgba, st.imnormal, st.grads["bg"], st.grads["textures"])
    buf, first = _carve([t.numel() * 4 for t in like], offsets, st.dev)
    N = pkg._native
    views = {}
    for name, t, f in zip(names, like, first):
        views[name] = buf[f:f + t.numel()]
        assert (views[name].data_ptr() % 256) == offsets[names.index(name)]
    st.d.rgba, st.d.imnormal = N.ptr(views["rgba"]), N.ptr(views["imnormal"])
    st.g.grad_bg, st.g.grad_textures = N.ptr(views["grad_bg"]), N.ptr(views["grad_textures"])
    assert st.step_mode_taken() == step_mode
    st.run()
    torch.cuda.synchronize()
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=st.dev)
    for name, t, f in zip(names, like, first):
        got = buf[f:f + t.numel()]
        inside[f:f + t.numel()] = True
        assert torch.equal(got, _bits(want[name]).reshape(-1)), name
    assert bool((buf[~inside] == SENTINEL).all()), "a guard word was written"
    assert int((~inside).sum()) >= 5 * 64
    for k, v in _results(st).items():                            # (everything that stayed where it was: the same step)
        if k not in names:
            assert torch.equal(_bits(v), _bits(want[k])), k


@pytest.mark.parametrize("tex", [(48, 40), (33, 65)], ids=["48x40", "33x65"])
def test_ragged_textures(pkg, tex):
    """texture sizes that are no multiple of the 32-texel tile, one with a width that is no multiple of 4 (the one-texel-per-lane store)"""
    new, old = _pair(pkg, "sphere", 3, 32, seed=45, tex=tex)
    a, b = _arrays(new), _arrays(old)
    _same(a, b)
    assert a["grad_textures"].shape[2:] == tex and float(a["grad_textures"].abs().max()) > 0


def test_texture_tiles_without_records_and_overflowing_ones(pkg):
    """Every face's uvs on the corner four texture tiles share, in a 72x100 texture of 3 x 4 tiles: eight tiles receive no record and are
    written as zeros all the same; the two close-ups overflow the record pool and are NaN in EVERY texel, the empty tiles' included, with the
    same payload on both paths."""
    kw = dict(seed=12, dist=[1.9, 1.9, 6.5], uv_corner=True, tex=(72, 100))
    new, old = _pair(pkg, "sphere", 3, 32, **kw)
    a, b = _arrays(new), _arrays(old)
    dn, do = new.dropped_records(), old.dropped_records()
    assert dn[0] > 0 and dn[1] > 0 and dn[2] == 0 and [x > 0 for x in dn] == [x > 0 for x in do]
    gn, go = a.pop("grad_textures"), b.pop("grad_textures")
    assert bool(torch.isnan(gn[:2]).all()) and bool(torch.isnan(go[:2]).all()) and bool(torch.isfinite(gn[2]).all())
    assert torch.equal(_bits(gn), _bits(go))
    touched = torch.zeros(72, 100, dtype=torch.bool, device=gn.device)
    touched[:64, :64] = True
    assert float(gn[2][:, touched].abs().max()) > 0 and float(gn[2][:, ~touched].abs().max()) == 0
    _same(a, b)


@pytest.mark.parametrize("B", [1, 9])
def test_small_batches_of_mostly_empty_tiles(pkg, B):
    """A far camera: most tiles take the four-tiles-per-wave path, whose last group of an image is partial.  B = 1, and B = 9 = 8 + 1 (both
    branches of the workgroup -> image mapping)."""
    new, old = _pair(pkg, "sphere", B, 40, ratio=0.6, seed=47, dist=8.0)
    a = _arrays(new)
    _same(a, _arrays(old))
    covered = (a["face_idx"] >= 0).float().mean()
    assert 0 < float(covered) < 0.5 and float(a["grad_bg"].abs().max()) > 0


def test_render_views_shares_the_stores(pkg):
    case = vw.Case(pkg, "sphere", 4, 64, 2, seed=5)
    v, r = case.render_both()
    case.check_forward(v, r)
    vw._backward_both(case, v, r, seed=17)
    case.check_grads("views")


def test_render_indexed_shares_the_stores(pkg):
    case = ix.Case(pkg, 11, ix.MIXED_ROWS, ix.MIXED, seed=7)
    v, g = case.render_indexed(), case.render_gathered()
    case.check_forward(v, g)
    ix._backward_both(case, v, g, seed=11)
    case.check_grads("mixed")
