"""DiffRender.render_views on the GPU: B samples x N views in one pass over B*N images that reads every sample's vertices, textures,
lights and bg from their single copy.

The reference everywhere below is ``DiffRender.render`` on EXPLICITLY REPLICATED leaf tensors (repeat_interleave(N, 0)): the path the rest
of the suite holds to the oracle -- never render_views itself.  Forward outputs must be bit-identical; per-view camera gradients too; the
gradient of a per-sample tensor must be, to the bit, the replicated path's (B*N,...) leaf gradient viewed (B,N,...) and added in ascending
view order in fp32 on the device.  One test anchors the whole against the CPU oracle at the suite's bars, so that the file does not only
compare the project with itself."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import TEMPLATES
from parity_bar import grad_close

pytestmark = pytest.mark.gpu
SHARED = ("vertices", "textures", "lights", "bg")
CAMERAS = ("azimuths", "elevations", "distances", "biases")


def _view_cameras(att, n, only_azimuths):
    """per-view cameras (B,n) / (B,n,2) around the sample's own: a turntable in azimuth, small steps in the rest"""
    k = torch.arange(n, dtype=torch.float32)
    cams = {"azimuths": att["azimuths"][:, None] + k[None] * (360.0 / max(n, 2)) + 7.0 * k[None] ** 2}
    if only_azimuths:
        cams.update({c: att[c] for c in CAMERAS[1:]})
    else:
        cams["elevations"] = att["elevations"][:, None] + 2.5 * k[None]
        cams["distances"] = att["distances"][:, None] * (1.0 + 0.06 * k[None])
        cams["biases"] = att["biases"][:, None, :] + 0.03 * k[None, :, None] * torch.tensor([1.0, -1.0])[None, None]
    return cams


class Case:
    """the two paths on the same numbers: `views` holds the (B,...) leaves render_views takes, `rep` the replicated (B*N,...) leaves of render"""

    def __init__(self, pkg, name, B, S, n, ratio=1, no_mask=True, seed=0, options=0, imn=True, only_azimuths=False, knobs=None):
        self.dev = dev = torch.device("cuda:0")
        self.dr = dr = pkg.DiffRender(os.path.join(TEMPLATES, name + ".npz"), S, ratio=ratio, emit_imnormal=imn)
        dr.options = options
        for k, v in (knobs or {}).items():
            setattr(dr, k, v)
        self.B, self.n, self.no_mask = B, n, no_mask
        self.H, self.W = dr.render_height, dr.image_size
        att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, B, self.H, self.W, seed=seed)
        self.att, self.gt = att, gt
        cams = _view_cameras(att, n, only_azimuths)
        self.view_axis = {c: cams[c].dim() == (3 if c == "biases" else 2) for c in CAMERAS}
        self.views = {k: att[k].to(dev).requires_grad_(True) for k in SHARED}
        self.views.update({c: cams[c].to(dev).contiguous().requires_grad_(True) for c in CAMERAS})
        self.rep = {k: att[k].to(dev).repeat_interleave(n, 0).contiguous().requires_grad_(True) for k in SHARED}
        for c in CAMERAS:
            full = cams[c] if self.view_axis[c] else cams[c].unsqueeze(1).expand((B, n) + tuple(cams[c].shape[1:]))
            self.rep[c] = full.reshape((B * n,) + tuple(full.shape[2:])).to(dev).contiguous().requires_grad_(True)
        if not no_mask:
            self.views["bg"] = self.rep["bg"] = None

    def render_both(self):
        rv, av = self.dr.render_views(no_mask=self.no_mask, **self.views)
        fv = self.dr.last_face_idx
        rr, ar = self.dr.render(no_mask=self.no_mask, **self.rep)
        fr = self.dr.last_face_idx
        return (rv, av, fv), (rr, ar, fr)

    def upstream(self, seed):
        g = torch.Generator().manual_seed(seed)
        w = torch.randn(self.B, self.n, 4, self.H, self.W, generator=g).to(self.dev)
        wfn = torch.randn(self.B, self.n, self.dr.num_faces, 3, generator=g).to(self.dev)
        return w, wfn

    def leaves(self):
        return [k for k in SHARED + CAMERAS if self.views[k] is not None]

    def zero_grads(self):
        for d in (self.views, self.rep):
            for t in d.values():
                if t is not None:
                    t.grad = None

    def check_forward(self, v, r):
        (rv, av, fv), (rr, ar, fr) = v, r
        B, n, H, W = self.B, self.n, self.H, self.W
        assert rv.shape == (B, n, 4, H, W) and rv.stride() == (n * H * W * 4, H * W * 4, 1, W * 4, 4)        # the permuted view of (B,N,H,W,4) memory
        assert fv.shape == (B, n, H, W) and av["face_normals"].shape == (B, n, self.dr.num_faces, 3)
        assert torch.equal(rv.detach().reshape(B * n, 4, H, W), rr.detach())
        assert torch.equal(fv.reshape(B * n, H, W), fr)
        assert float((fv >= 0).float().mean()) > 0.02
        assert torch.equal(av["face_normals"].detach().reshape(B * n, -1, 3), ar["face_normals"].detach())
        if self.dr.emit_imnormal:
            assert av["imnormal"].shape == (B, n, H, W, 3) and torch.equal(av["imnormal"].reshape(B * n, H, W, 3), ar["imnormal"])
        else:
            assert av["imnormal"] is None and ar["imnormal"] is None

    def check_grads(self, what="", keys=None):
        """the views path's gradients (of `keys`; default: every leaf) against the replicated path's leaf gradients"""
        B, n = self.B, self.n
        for k in keys or self.leaves():
            got, ref = self.views[k].grad, self.rep[k].grad
            assert got is not None and ref is not None, (what, k)
            ref = ref.reshape((B, n) + tuple(ref.shape[1:]))
            assert float(ref.abs().max()) > 0, (what, k)
            if k in CAMERAS and self.view_axis[k]:
                assert torch.equal(got, ref), (what, k)                                           # per view: the replicated path's bits
            elif k in CAMERAS:                                                                    # broadcast over the views: autograd's expand sums them
                if n <= 2:
                    assert torch.equal(got, ref[:, 0] + ref[:, 1] if n == 2 else ref[:, 0]), (what, k)
                else:
                    grad_close(got, ref.double().sum(1), what="%s %s (broadcast camera, torch's own reduction)" % (what, k))
            else:
                acc = ref[:, 0].clone()
                for v in range(1, n):
                    acc = acc + ref[:, v]                                                         # ((g0 + g1) + g2) + ... in fp32 on the device
                assert torch.equal(got, acc), (what, k, float((got - acc).abs().max()), float(acc.abs().max()))


def _backward_both(case, v, r, seed):
    (rv, av, _), (rr, ar, _) = v, r
    B, n, H, W = case.B, case.n, case.H, case.W
    w, wfn = case.upstream(seed)
    ((rv * w).sum() + (av["face_normals"] * wfn).sum()).backward()
    ((rr * w.reshape(B * n, 4, H, W)).sum() + (ar["face_normals"] * wfn.reshape(B * n, -1, 3)).sum()).backward()
    torch.cuda.synchronize()


CASES = [
    # label, template, B, S, N, ratio, no_mask, options (names of _native.OPT_*), emit_imnormal, only azimuths carry N
    ("config 1, N=1", "sphere", 4, 64, 1, 1, True, (), True, False),
    ("config 1, N=2", "sphere", 4, 64, 2, 1, True, (), True, False),
    ("config 1, N=5", "sphere", 4, 64, 5, 1, True, (), True, False),
    ("config 1, N=5, white background, no imnormal", "sphere", 4, 64, 5, 1, False, (), False, False),
    ("the trainer's Ae / Ae90 pair: 96 images", "smpl_uv_642", 48, 128, 2, 1, True, (), True, False),
    ("Market 128x64, N=3", "smpl_uv_642", 6, 64, 3, 2, True, (), True, False),
    ("Market 128x64, N=3, white background", "smpl_uv_642", 6, 64, 3, 2, False, (), True, False),
    ("options: strict cull, half-open boxes, xyz bands, one-wave walk", "sphere", 4, 64, 3, 1, True,
     ("OPT_CULL_STRICT", "OPT_BBOX_HALF_OPEN", "OPT_SH_ORDER_XYZ", "OPT_WALK_WAVE"), True, False),
    ("a turntable: only azimuths carry N = 2", "sphere", 4, 64, 2, 1, True, (), False, True),
    ("a turntable: only azimuths carry N = 5", "sphere", 4, 64, 5, 1, True, (), True, True),
]


@pytest.mark.parametrize("label,name,B,S,n,ratio,no_mask,opts,imn,only_az", CASES, ids=[c[0] for c in CASES])
def test_views_match_the_replicated_render_bit_for_bit(pkg, label, name, B, S, n, ratio, no_mask, opts, imn, only_az):
    options = 0
    for o in opts:
        options |= getattr(pkg._native, o)
    case = Case(pkg, name, B, S, n, ratio=ratio, no_mask=no_mask, seed=3 + n, options=options, imn=imn, only_azimuths=only_az)
    v, r = case.render_both()
    case.check_forward(v, r)
    _backward_both(case, v, r, seed=17)
    case.check_grads(label)
    if not no_mask:
        assert "bg" not in case.leaves()


def test_non_default_rasteriser_constants_pass_through(pkg):
    """knum, sigmainv, boxlen, multiplier, eps travel in the descriptor of the B*N images unchanged"""
    case = Case(pkg, "sphere", 3, 48, 3, seed=21, knobs=dict(knum=7, boxlen=0.08, sigmainv=900.0, eps=1e-7))
    v, r = case.render_both()
    case.check_forward(v, r)
    _backward_both(case, v, r, seed=5)
    case.check_grads("constants")


def test_anchor_against_the_oracle(pkg, oracle):
    """config 1, N = 2 against the CPU oracle on the replicated inputs, at the suite's bars: face_idx exact, RGBA 1e-4, gradients within 1e-4
    of their own maximum -- per view for the cameras, the oracle's per-image gradients summed over the views in float64 for the shared inputs."""
    B, n, S = 4, 2, 64
    case = Case(pkg, "sphere", B, S, n, seed=0)
    rv, av = case.dr.render_views(no_mask=True, **case.views)
    rng = np.random.default_rng(77)
    w = rng.normal(size=(B * n, S, S, 4)).astype(np.float32)
    wfn = rng.normal(size=(B * n, case.dr.num_faces, 3)).astype(np.float32)
    dev = case.dev
    ((rv.permute(0, 1, 3, 4, 2).reshape(B * n, S, S, 4) * torch.from_numpy(w).to(dev)).sum()
     + (av["face_normals"].reshape(B * n, -1, 3) * torch.from_numpy(wfn).to(dev)).sum()).backward()
    torch.cuda.synchronize()
    inp = {k: case.rep[k].detach().cpu().numpy() for k in SHARED + CAMERAS}
    inp["faces"] = case.dr.faces.numpy().astype(np.int32)
    inp["face_uvs"] = case.dr.face_uvs.numpy()[0]
    proj = case.dr.cam_proj.numpy().reshape(3)
    rgba_o, fidx_o, fn_o, imn_o = oracle.render_forward(inp, S, S, True, proj)
    assert (case.dr.last_face_idx.reshape(B * n, S, S).cpu().numpy() == fidx_o).all()
    assert (fidx_o >= 0).mean() > 0.03
    assert np.abs(rv.detach().permute(0, 1, 3, 4, 2).reshape(B * n, S, S, 4).cpu().numpy() - rgba_o).max() <= 1e-4
    assert np.abs(av["face_normals"].detach().reshape(B * n, -1, 3).cpu().numpy() - fn_o).max() <= 1e-6
    g_o = oracle.render_backward(inp, S, S, True, proj, w, wfn)
    g64 = {}

    def ref64(k):
        if not g64:
            g64.update(oracle.render_backward(inp, S, S, True, proj, w.astype(np.float64), wfn.astype(np.float64), dtype=np.float64))
        return g64[k]

    def fold(k, g):                                                     # the oracle's per-image gradient, as render_views returns it
        g = np.asarray(g)
        g = g.reshape((B, n) + g.shape[1:])
        return g.astype(np.float64).sum(1) if k in SHARED else g
    for k in SHARED + CAMERAS:
        ref = fold(k, g_o[k])
        assert float(np.abs(ref).max()) > 0.5, k
        verdict = grad_close(case.views[k].grad, ref, rtol=1e-4, what="anchor, " + k, ref64=lambda k=k: fold(k, ref64(k)))
        assert verdict == "ok", (k, verdict)


def test_two_backward_runs_of_one_graph_are_bit_identical(pkg):
    case = Case(pkg, "smpl_uv_642", 6, 128, 3, seed=9)
    rv, av = case.dr.render_views(no_mask=True, **case.views)
    w, wfn = case.upstream(4)
    loss = (rv * w).sum() + (av["face_normals"] * wfn).sum()
    runs = []
    for _ in range(2):
        case.zero_grads()
        loss.backward(retain_graph=True)
        torch.cuda.synchronize()
        runs.append({k: case.views[k].grad.clone() for k in case.leaves()})
    for k in runs[0]:
        assert float(runs[0][k].abs().max()) > 0 and torch.equal(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("n", [2, 3])
def test_recon_data_on_a_view_slice(pkg, n):
    """render_views -> recon_data(rgbs[:, 0], gt) + rgbs[:, 1, :3].mean() -> backward: the loss's bits and every gradient against the same
    expression on the replicated render's image, viewed (B,N,4,H,W)"""
    case = Case(pkg, "sphere", 4, 64, n, seed=31)
    v, r = case.render_both()
    gt = case.gt.to(case.dev)
    B, H, W = case.B, case.H, case.W
    rv, rr = v[0], r[0].reshape(B, n, 4, H, W)
    lv = case.dr.recon_data(rv[:, 0], gt, no_mask=True) + rv[:, 1, :3].mean()
    lr = case.dr.recon_data(rr[:, 0], gt, no_mask=True) + rr[:, 1, :3].mean()
    assert torch.equal(lv.detach(), lr.detach()) and float(lv.detach()) > 0
    lv.backward()
    lr.backward()
    torch.cuda.synchronize()
    case.check_grads("recon_data on a slice")


def _overflowing_case(pkg, extra, check):
    """test_gpu_parity's record-overflow construction as 2 samples x 2 views: every face_uvs entry on the corner shared by four 32x32-texel tiles
    (four texture-gradient records per covered pixel against room for 9/8 per pixel), the sphere at distance 1.9 in every image"""
    case = Case(pkg, "sphere", 2, 64, 2, seed=12, knobs=dict(extra_texture_records_per_pixel=extra, check_texture_records=check))
    Ht, Wt = case.att["textures"].shape[2:]
    uv = torch.empty_like(case.dr.face_uvs)
    uv[..., 0] = 32.0 / Wt                                           # texel coordinates (31.5, 31.5)
    uv[..., 1] = 1.0 - 32.0 / Ht
    case.dr.face_uvs = uv
    with torch.no_grad():
        case.views["distances"].fill_(1.9)
        case.rep["distances"].fill_(1.9)
    return case


def test_texture_record_pool_overflow_through_render_views(pkg):
    """The record check of RenderViewsNode's backward, whose render workspace starts behind the staging head of the multi-view workspace: silent
    NaNs + the status word without the switch, the per-image counts in the message with it, and the replicated render's bits once the pool holds."""
    B, n = 2, 2
    case = _overflowing_case(pkg, 0.0, False)
    w, _ = case.upstream(8)
    rv, _ = case.dr.render_views(no_mask=True, **case.views)
    covered = (case.dr.last_face_idx >= 0).float().mean(dim=(2, 3))
    assert covered.shape == (B, n) and float(covered.min()) > 0.4      # 4 x 0.4 HW records per image against room for 9/8 HW
    (rv * w).sum().backward()
    torch.cuda.synchronize()
    assert torch.isnan(case.views["textures"].grad).all()           # every sample: a NaN of one view's survives the sum over the views
    assert case.dr.poll_dropped_records(reset=False) > 0
    with pytest.raises(RuntimeError, match="dropped"):
        case.dr.render_views(no_mask=True, **{k: v.detach() for k, v in case.views.items()})

    case = _overflowing_case(pkg, 0.0, True)
    rv, _ = case.dr.render_views(no_mask=True, **case.views)
    with pytest.raises(RuntimeError, match="texture-record pool") as err:
        (rv * w).sum().backward()
    counts = [int(c) for c in re.search(r"\[([^\]]*)\]", str(err.value)).group(1).split(",")]
    assert len(counts) == B * n and all(c > 0 for c in counts), str(err.value)

    case = _overflowing_case(pkg, 3.0, True)                        # 4 1/8 records per pixel: enough for any image
    v, r = case.render_both()
    case.check_forward(v, r)
    _backward_both(case, v, r, seed=8)
    case.check_grads("a record pool that holds")


def test_only_the_normals_are_differentiated(pkg):
    """loss = (face_normals * w).sum() alone: the image's gradient arrives undefined at the node, which then differentiates a zero image gradient --
    vertices and cameras get the replicated render's bits, textures, lights and bg exact zeros; render_geometry, which has no image at all, gives
    the same bits as that render (test_gpu_parity's geometry-only test compares the two to 1e-6 of the maximum)"""
    case = Case(pkg, "smpl_uv_642", 2, 64, 3, seed=41)
    (_, av, _), (_, ar, _) = case.render_both()
    _, wfn = case.upstream(6)
    wfn_rep = wfn.reshape(case.B * case.n, -1, 3)
    (av["face_normals"] * wfn).sum().backward()
    (ar["face_normals"] * wfn_rep).sum().backward()
    torch.cuda.synchronize()
    geometry = ("vertices",) + CAMERAS
    case.check_grads("normals only", keys=geometry)
    for k in ("textures", "lights", "bg"):
        for leaf in (case.views[k], case.rep[k]):
            assert leaf.grad is not None and leaf.grad.shape == leaf.shape and int(torch.count_nonzero(leaf.grad)) == 0, k
    geo = {k: case.rep[k].detach().clone().requires_grad_(True) for k in case.rep}
    out = case.dr.render_geometry(**geo)
    assert torch.equal(out["face_normals"].detach(), ar["face_normals"].detach())
    (out["face_normals"] * wfn_rep).sum().backward()
    torch.cuda.synchronize()
    for k in geometry:
        assert torch.equal(geo[k].grad, case.rep[k].grad), (k, float((geo[k].grad - case.rep[k].grad).abs().max()))
    assert all(geo[k].grad is None for k in ("textures", "lights", "bg"))


def test_broadcast_cameras_get_gradients_of_their_own_shapes(pkg):
    """elevations, distances (B,) and biases (B,2) next to azimuths (B,N): every gradient has its leaf's shape and is, N being 2, the sum over the
    views of the gradient the same call gives with every camera spelled out as (B,N) / (B,N,2) (two addends: no order to differ in)"""
    B, n = 3, 2
    case = Case(pkg, "sphere", B, 64, n, seed=23, only_azimuths=True)
    assert [tuple(case.views[c].shape) for c in CAMERAS] == [(B, n), (B,), (B,), (B, 2)]
    full = {k: v.detach().clone().requires_grad_(True) for k, v in case.views.items()}
    for c in CAMERAS[1:]:
        t = case.views[c].detach()
        full[c] = t.unsqueeze(1).expand((B, n) + tuple(t.shape[1:])).contiguous().requires_grad_(True)
    w, wfn = case.upstream(13)
    for leaves in (case.views, full):
        rv, av = case.dr.render_views(no_mask=True, **leaves)
        ((rv * w).sum() + (av["face_normals"] * wfn).sum()).backward()
    torch.cuda.synchronize()
    for k in case.leaves():
        got, ref = case.views[k].grad, full[k].grad
        assert got.shape == case.views[k].shape and ref.shape == full[k].shape and float(ref.abs().max()) > 0, k
        assert torch.equal(got, ref[:, 0] + ref[:, 1] if k in CAMERAS[1:] else ref), k


def test_no_host_synchronisation(pkg):
    case = Case(pkg, "sphere", 4, 64, 3, seed=2)
    w, wfn = case.upstream(1)
    rv, av = case.dr.render_views(no_mask=True, **case.views)       # (the shape's first call: library, extension and descriptor caches are warm after it)
    ((rv * w).sum() + (av["face_normals"] * wfn).sum()).backward()
    case.zero_grads()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            torch.ones(1, device=case.dev).item()
            raised = False
        except RuntimeError:
            raised = True
        if not raised:
            pytest.skip("this torch build does not raise on a synchronising call under set_sync_debug_mode('error')")
        rv, av = case.dr.render_views(no_mask=True, **case.views)
        ((rv * w).sum() + (av["face_normals"] * wfn).sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert all(torch.isfinite(case.views[k].grad).all() for k in case.leaves())


def test_nothing_is_replicated_on_the_way_in(pkg):
    """config 2 (B = 48, 128x128, texture 256x128) with N = 36 under no_grad: what the call allocates beyond its returned tensors and its
    workspace stays below ONE replicated texture tensor (B*N*3*Ht*Wt*4 bytes) -- the replicated path exceeds that by construction."""
    B, n, S = 48, 36, 128
    N = pkg._native
    dev = torch.device("cuda:0")
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "smpl_uv_642.npz"), S)
    att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, B, S, S, seed=0)
    a = {k: att[k].to(dev) for k in SHARED + CAMERAS}
    a["azimuths"] = (a["azimuths"][:, None] + torch.arange(n, device=dev, dtype=torch.float32)[None] * 10.0).contiguous()
    Ht, Wt = a["textures"].shape[2:]
    with torch.no_grad():
        small = {k: v[:1].contiguous() for k, v in a.items()}
        dr.render_views(no_mask=True, **small)                         # loads the library and the extension outside the measurement
        del small
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        rgbs, out = dr.render_views(no_mask=True, **a)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated(dev) - before
    vd = N.MMRenderViewsDesc()
    proto = dr._proto(dr._static(dev), B * n, True, Ht, Wt)[0]
    ctypes.memmove(ctypes.byref(vd), proto, len(proto))
    vd.views = n
    workspace = int(N.lib().mm_render_views_query_workspace(ctypes.byref(vd)))
    returned = sum(t.numel() * t.element_size() for t in (rgbs, out["face_normals"], out["imnormal"], dr.last_face_idx))
    assert rgbs.shape == (B, n, 4, S, S) and returned >= B * n * S * S * 4 * 4
    one_replicated_texture = B * n * 3 * Ht * Wt * 4
    assert rise - returned - workspace < one_replicated_texture, (rise, returned, workspace, one_replicated_texture)
    assert rise >= returned                                             # (the measurement saw the call)
