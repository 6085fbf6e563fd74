"""The kaolin-shaped operators of 3d-magic-mirror_amd/shim at their edges, reached through kaolin's own module paths.

tests/test_gpu_shim_ops.py runs each operator at one or two small shapes, mostly against the C oracle, which evaluates the same
expressions as the kernels.  Here every operator that torch can express is held to a float64 CPU restatement of what kaolin
does, differentiated by torch autograd, at the shapes where kernels go wrong:
exact rounding ties and border coordinates, sizes of one, sizes that straddle the kernels' unrolls, trips and lane counts,
degenerate inputs and the branches for inputs that take no part in the gradient.  dibr_rasterization is held to the oracle here
(face_idx bit-exact, values, gradients with the float64 oracle as the conditioning referee); its torch form -- decisions by brute force,
the derivative autograd's -- is tests/render_ref.py, which tests/test_gpu_render_ref.py holds the whole operator chain to.
Bars: values within 1e-4 on the max(1, |ref|) scale; gradients within 1e-4 of the reference's own maximum (tests/parity_bar.py);
equality where the kernel is exact."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn

from conftest import ROOT, TEMPLATES, make_inputs
from parity_bar import grad_close

pytestmark = pytest.mark.gpu
SHIM = os.path.join(ROOT, "3d-magic-mirror_amd", "shim")
DEV = torch.device("cuda:0")
LEAVES = ("vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases")


@pytest.fixture(scope="module")
def kal():
    if SHIM not in sys.path:
        sys.path.insert(0, SHIM)
    import kaolin
    return kaolin


def _np(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def _close(got, ref, tol=1e-4, what=""):
    """values: max|got - ref| <= tol * max(1, max|ref|)"""
    got, ref = _np(got), _np(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    assert err <= tol * scale, (what, err, scale)


def _gclose(got, ref, tol=1e-4, what="", ref64=None):
    """gradients: relative to the reference's own maximum, no floor (tests/parity_bar.py)"""
    grad_close(_np(got), _np(ref), rtol=tol, what=what, ref64=ref64)


def _leaf(a, dtype=torch.float32, grad=True):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).requires_grad_(grad)


def _ref_leaf(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(torch.float64).requires_grad_(True)


# ---------------------------------------------------------------------------------------------------------------------
# texture_mapping: F.grid_sample(tex, (2u - 1, -(2v - 1)), mode, align_corners=False, padding_mode='border') in float64
# ---------------------------------------------------------------------------------------------------------------------
def _tex_ref(uv, tex, mode):
    """uv (B,N,2), tex (B,C,Ht,Wt), float64 CPU -> (B,N,C)"""
    grid = torch.stack([uv[..., 0] * 2 - 1, -(uv[..., 1] * 2 - 1)], -1).unsqueeze(2)
    return Fnn.grid_sample(tex, grid, mode=mode, align_corners=False, padding_mode="border")[..., 0].permute(0, 2, 1)


def _dyadic_uv(g, shape, lo=-0.25, hi=1.25, bits=16):
    """coordinates on the 2^-bits grid: every step of the kernels' unnormalisation is exact in fp32 for the texture sizes used
    here, so fp32 and fp64 land on the same side of every texel boundary and of every nearest-mode tie"""
    k = torch.randint(int(lo * 2 ** bits), int(hi * 2 ** bits) + 1, shape, generator=g)
    return k.double() / 2 ** bits


def _tex_case(kal, uv, tex, mode, dout, want_uv=True, want_tex=True, shared=False, what=""):
    """run the operator (fp32) and the float64 reference on the same inputs; compare values and the requested gradients"""
    B = uv.shape[0]
    uvd = uv.float().to(DEV).requires_grad_(want_uv)
    texd = tex.float().to(DEV).requires_grad_(want_tex)
    out = kal.render.mesh.texture_mapping(uvd, texd, mode=mode)
    uvr, texr = uv.double().requires_grad_(want_uv), tex.double().requires_grad_(want_tex)
    texr_b = texr.unsqueeze(0).expand(B, -1, -1, -1) if shared else texr
    ref = _tex_ref(uvr.reshape(B, -1, 2), texr_b, mode).reshape(out.shape)
    if mode == "nearest":
        assert torch.equal(out.cpu().double(), ref.detach()), what          # a copy of one texel: exact
    else:
        _close(out, ref, 1e-5, what)
    out.backward(dout.float().to(DEV))
    ref.backward(dout.double())
    if want_uv:
        if mode == "nearest":
            assert torch.equal(uvd.grad, torch.zeros_like(uvd)), what       # piecewise constant: exactly zero
        else:
            _gclose(uvd.grad, uvr.grad, what=what + " d/duv")
            assert (uvd.grad.cpu()[uvr.grad == 0] == 0).all(), what        # clamped axes (the border rule) give exact zeros
    else:
        assert uvd.grad is None
    if want_tex:
        _gclose(texd.grad, texr.grad, what=what + " d/dtex")
    else:
        assert texd.grad is None
    return out, uvd, texd, uvr, texr


def _exact_axis(n):
    """coordinates (in [0,1] units along an axis of n texels) at the edges of the unnormalisation ix = u * n - 0.5"""
    e = 2.0 ** -20
    pts = [0.5 / n, 1 - 0.5 / n]                                   # ix = 0 and ix = n - 1 exactly
    pts += [(k + 0.5) / n for k in range(n)]                       # integer ix
    pts += [k / n for k in range(n + 1)]                           # half-integer ix: nearest-mode ties
    pts += [e, 1 - e, -e, 1 + e, 0.0, 1.0, -3.0, 4.5]              # just inside / outside [0,1], far outside
    return torch.tensor(sorted(set(pts)), dtype=torch.float64)


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_texture_mapping_exact_coordinates_ties_and_borders(kal, mode):
    """Power-of-two maps (Ht != Wt): every coordinate below is exact in fp32 and fp64.  Nearest mode rounds ties half to even
    (std::nearbyint, as ATen); bilinear at integer ix and at the exact borders ix = 0 / ix = W-1 follows ATen's clip rule
    (a zero coordinate gradient on the border itself)."""
    g = torch.Generator().manual_seed(11)
    B, C, Ht, Wt = 2, 3, 4, 8
    us, vs = _exact_axis(Wt), _exact_axis(Ht)
    uu, vv = torch.meshgrid(us, vs, indexing="ij")
    uv = torch.stack([uu.reshape(-1), vv.reshape(-1)], -1)[None].repeat(B, 1, 1)
    tex = torch.rand(B, C, Ht, Wt, generator=g, dtype=torch.float64).float().double()
    dout = torch.randn(B, uv.shape[1], C, generator=g, dtype=torch.float64).float().double()
    _tex_case(kal, uv, tex, mode, dout, what="exact coordinates, " + mode)
    # the ties alone, nearest: the texel index is the even neighbour (a mistaken round-half-away picks the odd one at half of them)
    if mode == "nearest":
        ties = torch.tensor([[(k + 1) / Wt, (j + 1) / Ht] for k in range(Wt - 1) for j in range(Ht - 1)], dtype=torch.float64)[None]
        ramp = torch.arange(Ht * Wt, dtype=torch.float64).reshape(1, 1, Ht, Wt)
        out = kal.render.mesh.texture_mapping(ties.float().cuda(), ramp.float().cuda(), mode="nearest").cpu().double()[0, :, 0]
        ix = (ties[0, :, 0] * Wt - 0.5).round()                  # torch.round: half to even
        iy = ((1 - ties[0, :, 1]) * Ht - 0.5).round()
        assert torch.equal(out, iy * Wt + ix)


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("C,Ht,Wt,shared", [
    (1, 1, 1, False), (4, 1, 8, False), (16, 8, 1, False), (4, 16, 64, True), (1, 32, 8, True), (16, 12, 40, False)])
def test_texture_mapping_texture_shapes(kal, mode, C, Ht, Wt, shared):
    """maps of one texel along an axis, one / four / sixteen channels, Ht != Wt (one not a power of two), a shared (C,Ht,Wt) map"""
    g = torch.Generator().manual_seed(C * 1000 + Ht * 10 + Wt)
    B, H, W = 3, 9, 13
    uv = _dyadic_uv(g, (B, H, W, 2), -0.3, 1.3)
    tex = torch.rand((C, Ht, Wt) if shared else (B, C, Ht, Wt), generator=g).double()
    dout = torch.randn(B, H, W, C, generator=g).double()
    out = _tex_case(kal, uv, tex, mode, dout, shared=shared, what="C=%d %dx%d shared=%s %s" % (C, Ht, Wt, shared, mode))[0]
    assert out.shape == (B, H, W, C)


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("want", ["uv", "tex"])
def test_texture_mapping_single_input_gradients(kal, mode, want):
    """only the coordinates, or only the texture, require grad: the other gradient is never formed"""
    g = torch.Generator().manual_seed(3)
    B, N, C, Ht, Wt = 2, 777, 3, 16, 32
    uv = _dyadic_uv(g, (B, N, 2))
    tex = torch.rand(B, C, Ht, Wt, generator=g).double()
    dout = torch.randn(B, N, C, generator=g).double()
    _tex_case(kal, uv, tex, mode, dout, want_uv=want == "uv", want_tex=want == "tex", what="%s only, %s" % (want, mode))


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_texture_mapping_large_batches_pile_ups_and_strided_passes(kal, mode):
    """512x512 coordinates, B = 4, C*Ht*Wt = 131072 texels: the fixed-point scatter's max pass (8 workgroups) and finish pass
    (256 workgroups) both stride; a quarter of every image's points pile onto one texel"""
    g = torch.Generator().manual_seed(4)
    B, C, Ht, Wt = 4, 4, 128, 256
    uv = _dyadic_uv(g, (B, 512, 512, 2), -0.1, 1.1, bits=14)
    uv[:, :128] = torch.tensor([37.5 / Wt, 1 - 90.5 / Ht], dtype=torch.float64)     # a texel centre (bilinear: one texel of weight 1)
    tex = torch.rand(B, C, Ht, Wt, generator=g).double()
    dout = torch.randn(B, 512, 512, C, generator=g).double()
    _tex_case(kal, uv, tex, mode, dout, what="large N, " + mode)


def test_texture_mapping_small_contributions_keep_their_precision_next_to_a_huge_one(kal):
    """The texture gradient is accumulated per image in 64-bit fixed point scaled to that image's largest |upstream value|.  One
    value 1e6 times the rest: every texel it does not touch must still match float64 element by element to 1e-4 relative (the
    coordinates sit on quarter texels, so every bilinear weight is a multiple of 1/16 and no texel gets a vanishing share)."""
    g = torch.Generator().manual_seed(6)
    B, C, Ht, Wt, N = 2, 2, 16, 16, 4096
    ix = torch.randint(0, 4 * (Wt - 1), (B, N), generator=g).double() / 4
    iy = torch.randint(0, 4 * (Ht - 1), (B, N), generator=g).double() / 4
    uv = torch.stack([(ix + 0.5) / Wt, 1 - (iy + 0.5) / Ht], -1)
    tex = torch.rand(B, C, Ht, Wt, generator=g).double()
    dout = (torch.rand(B, N, C, generator=g) * 0.5 + 0.5).double()
    dout[0, 5, 0] = 1e6 * float(dout[0, 5, 0])
    uvd, texd = uv.float().cuda(), tex.float().cuda().requires_grad_(True)
    kal.render.mesh.texture_mapping(uvd, texd, mode="bilinear").backward(dout.float().cuda())
    texr = tex.clone().requires_grad_(True)
    _tex_ref(uv, texr, "bilinear").backward(dout)
    got, ref = texd.grad.cpu().double(), texr.grad
    # the texels the big value reaches
    big = torch.zeros_like(ref, dtype=torch.bool)
    x0, y0 = int(ix[0, 5].floor()), int(iy[0, 5].floor())
    big[0, 0, y0:y0 + 2, x0:x0 + 2] = True
    rel = ((got - ref).abs() / ref.abs().clamp_min(1e-300))[~big]
    assert float(rel.max()) <= 1e-4, float(rel.max())
    assert torch.equal(got[ref == 0], ref[ref == 0])
    assert float(((got - ref).abs() / ref.abs())[big & (ref != 0)].max()) <= 1e-4


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64, "strided"])
@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_texture_mapping_dtypes_and_layouts_are_the_fp32_call(kal, mode, dtype):
    """fp16 / bf16 / fp64 inputs and non-contiguous coordinates: the values are, bit for bit, those of the fp32 call on the
    contiguous fp32 copies, and the gradients are that call's bits cast to the input's dtype"""
    g = torch.Generator().manual_seed(8)
    B, H, W, C, Ht, Wt = 2, 12, 20, 3, 16, 8
    dt = torch.float32 if dtype == "strided" else dtype
    uv = (torch.rand(B, H, W, 2, generator=g) * 1.2 - 0.1).to(dt)
    tex = torch.rand(B, C, Ht, Wt, generator=g).to(dt)
    dout = torch.randn(B, H, W, C, generator=g)
    if dtype == "strided":                                          # (B,2,H,W) permuted and (B,H,W,3) sliced coordinates
        uvs = [uv.permute(0, 3, 1, 2).contiguous().cuda().permute(0, 2, 3, 1),
               torch.cat([uv, uv[..., :1]], -1).cuda()[..., :2]]
    else:
        uvs = [uv.cuda()]
    uv32 = uv.float().cuda().requires_grad_(True)
    tex32 = tex.float().cuda().requires_grad_(True)
    out32 = kal.render.mesh.texture_mapping(uv32, tex32, mode=mode)
    out32.backward(dout.cuda())
    for u in uvs:
        assert dtype != "strided" or not u.is_contiguous()
        ud = u.detach().requires_grad_(True)
        td = tex.cuda().requires_grad_(True)
        out = kal.render.mesh.texture_mapping(ud, td, mode=mode)
        assert out.dtype == torch.float32 and torch.equal(out, out32)
        out.backward(dout.cuda())
        assert ud.grad.dtype == dt and torch.equal(ud.grad, uv32.grad.to(dt))
        assert td.grad.dtype == dt and torch.equal(td.grad, tex32.grad.to(dt))


# ---------------------------------------------------------------------------------------------------------------------
# spherical_harmonic_lighting: SURVEY a10's band order and constants
# ---------------------------------------------------------------------------------------------------------------------
def _sh_ref(n, L):
    x, y, z = n.unbind(-1)
    bands = torch.stack([torch.full_like(x, 0.28209479), 0.48860251 * x, 0.48860251 * z, 0.48860251 * y, 1.09254843 * x * y,
                         1.09254843 * y * z, 0.94617470 * z * z - 0.31539157, 0.77254840 * x * z, 0.38627420 * (x * x - y * y)], -1)
    return (bands * L[:, None, :]).sum(-1)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", [1, 255, 1025, 8192, 8193, 3 * 8192 + 17, 512 * 512])
def test_spherical_harmonic_lighting_sizes_straddling_the_light_gradient_trips(kal, B, N):
    """N across the light-gradient kernel's unroll (8 points per thread) and trips (1024 x 8 points): unit normals, normals of
    length up to 3, rows of zero normals (uncovered pixels)"""
    g = torch.Generator().manual_seed(B * 7 + N)
    n = torch.randn(B, N, 3, generator=g)
    n[:, ::2] = n[:, ::2] / n[:, ::2].norm(dim=-1, keepdim=True)
    n[:, 1::2] *= 1.5
    n[:, ::7] = 0
    L = torch.randn(B, 9, generator=g)
    dc = torch.randn(B, N, generator=g)
    nd, Ld = n.cuda().requires_grad_(True), L.cuda().requires_grad_(True)
    out = kal.render.mesh.spherical_harmonic_lighting(nd, Ld)
    nr, Lr = n.double().requires_grad_(True), L.double().requires_grad_(True)
    ref = _sh_ref(nr, Lr)
    _close(out, ref, what="sh values")
    out.backward(dc.cuda()); ref.backward(dc.double())
    _gclose(nd.grad, nr.grad, what="sh d/dnormals")
    _gclose(Ld.grad, Lr.grad, what="sh d/dlights")


@pytest.mark.parametrize("want", ["normals", "lights"])
def test_spherical_harmonic_lighting_single_input_gradients(kal, want):
    g = torch.Generator().manual_seed(12)
    B, H, W = 3, 33, 65
    n = torch.randn(B, H, W, 3, generator=g)
    L = torch.randn(B, 9, generator=g)
    dc = torch.randn(B, H, W, generator=g)
    nd, Ld = n.cuda().requires_grad_(want == "normals"), L.cuda().requires_grad_(want == "lights")
    out = kal.render.mesh.spherical_harmonic_lighting(nd, Ld)
    nr, Lr = n.double().requires_grad_(want == "normals"), L.double().requires_grad_(want == "lights")
    ref = _sh_ref(nr.reshape(B, -1, 3), Lr).reshape(B, H, W)
    _close(out, ref)
    out.backward(dc.cuda()); ref.backward(dc.double())
    if want == "normals":
        _gclose(nd.grad, nr.grad, what="d/dnormals alone")
        assert Ld.grad is None
    else:
        _gclose(Ld.grad, Lr.grad, what="d/dlights alone")
        assert nd.grad is None


# ---------------------------------------------------------------------------------------------------------------------
# mask_iou: 1 - mean_b[ sum(l r) / (sum(l + r - l r) + 1e-10) ]
# ---------------------------------------------------------------------------------------------------------------------
def _iou_ref(a, b):
    B = a.shape[0]
    mul = a * b
    return 1.0 - torch.mean(mul.reshape(B, -1).sum(1) / (((a + b) - mul).reshape(B, -1).sum(1) + 1e-10))


def _iou_case(kal, a, b, upstream=1.0, want=("l", "r"), what=""):
    ad, bd = a.cuda().requires_grad_("l" in want), b.cuda().requires_grad_("r" in want)
    loss = kal.metrics.render.mask_iou(ad, bd)
    ar, br = a.double().requires_grad_("l" in want), b.double().requires_grad_("r" in want)
    ref = _iou_ref(ar, br)
    _close(loss, ref, what=what)
    (loss * upstream).backward(); (ref * upstream).backward()
    for got, r, k in ((ad, ar, "l"), (bd, br, "r")):
        if k in want:
            _gclose(got.grad, r.grad, what="%s d/d%s" % (what, k))
        else:
            assert got.grad is None
    return loss, ad, bd


@pytest.mark.parametrize("B,N", [(B, N) for B in (1, 63, 64, 65, 130) for N in (1, 1023, 1025)] + [(1, 512 * 512), (65, 512 * 512)])
def test_mask_iou_batches_across_the_fold_and_sizes_across_the_block(kal, B, N):
    """B across the final kernel's 64 lanes (it folds the images in strides of 64), N across the 1024-thread reduction; soft masks"""
    g = torch.Generator().manual_seed(B * 10007 + N)
    a = torch.rand(B, 1, N, generator=g)
    b = torch.rand(B, 1, N, generator=g)
    b[::3] = (b[::3] > 0.5).float()
    _iou_case(kal, a, b, upstream=-2.5, what="B=%d N=%d" % (B, N))


def test_mask_iou_empty_identical_and_disjoint_masks(kal):
    """an all-zero pair (union 0: that image's IoU is 0 and its gradient exactly 0), identical binary masks, disjoint masks and
    soft masks in one batch; lhs-only and rhs-only gradients; upstream gradients other than one"""
    g = torch.Generator().manual_seed(21)
    B, H, W = 6, 31, 47
    a = torch.rand(B, H, W, generator=g)
    b = torch.rand(B, H, W, generator=g)
    a[0] = 0; b[0] = 0                                              # empty union
    a[1] = (a[1] > 0.4).float(); b[1] = a[1]                        # identical
    a[2] = (a[2] > 0.5).float(); b[2] = 1 - a[2]                    # disjoint
    a[3] = a[3] * (a[3] > 0.6).float(); b[3] = b[3] * (b[3] < 0.3).float()   # soft masks with partial supports
    for upstream, want in ((1.0, ("l", "r")), (0.37, ("l",)), (-4.0, ("r",))):
        loss, ad, bd = _iou_case(kal, a, b, upstream, want, what="special masks %s" % (want,))
        for t in (ad, bd):
            if t.grad is not None:
                assert torch.equal(t.grad[0], torch.zeros_like(t.grad[0]))
    assert abs(float(kal.metrics.render.mask_iou(a[1:2].cuda(), b[1:2].cuda()))) < 1e-6
    assert abs(float(kal.metrics.render.mask_iou(a[2:3].cuda(), b[2:3].cuda())) - 1.0) < 1e-6
    assert float(kal.metrics.render.mask_iou(a[:1].cuda(), b[:1].cuda())) == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# face_normals: cross(v1 - v0, v2 - v0) [/ (|n| + 1e-10)]
# ---------------------------------------------------------------------------------------------------------------------
def _fn_ref(fv, unit):
    n = torch.cross(fv[..., 1, :] - fv[..., 0, :], fv[..., 2, :] - fv[..., 0, :], dim=-1)
    return n / (n.norm(dim=-1, keepdim=True) + 1e-10) if unit else n


def _fn_case(kal, fv, unit, what):
    fvd = fv.float().cuda().requires_grad_(True)
    out = kal.ops.mesh.face_normals(fvd, unit=unit)
    fvr = fv.double().requires_grad_(True)
    ref = _fn_ref(fvr, unit)
    assert out.shape == fv.shape[:-2] + (3,)
    _close(out, ref, 1e-5, what)
    w = torch.randn(ref.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    out.backward(w.float().cuda()); ref.backward(w)
    return out, fvd, fvr


@pytest.mark.parametrize("unit", [True, False])
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("lead", [(1,), (255,), (257,), (1000,), (2, 3, 129)])
def test_face_normals_scales_counts_and_leading_dims(kal, unit, scale, lead):
    rng = np.random.default_rng(len(lead) * 100 + lead[-1])
    n = int(np.prod(lead))
    a, b, c = rng.uniform(0.5, 1.5, n), rng.uniform(-1, 1, n), rng.uniform(0.5, 1.5, n)
    tri = np.stack([np.zeros((n, 3)), np.stack([a, 0 * a, 0 * a], -1), np.stack([b, c, 0 * a], -1)], 1)   # no sliver: fp32 stays well conditioned
    tri = tri @ _rotation(rng, n).transpose(0, 2, 1) + rng.normal(size=(n, 1, 3))
    fv = torch.from_numpy((tri * scale).astype(np.float32).reshape(lead + (3, 3))).double()
    out, fvd, fvr = _fn_case(kal, fv, unit, "scale %g %s unit=%s" % (scale, lead, unit))
    _gclose(fvd.grad, fvr.grad, what="face_normals d/dfv")


@pytest.mark.parametrize("unit", [True, False])
def test_face_normals_coincident_and_collinear_corners(kal, unit):
    """|n| = 0 exactly in fp32 and fp64 (dyadic coordinates): the normal is exactly zero, and the unit form's gradient is that of
    n / (|n| + 1e-10) with the norm's gradient taken as zero at 0 (torch's rule), i.e. g / 1e-10 pushed through the cross product"""
    g = torch.Generator().manual_seed(5)
    F = 300
    base = torch.randint(-64, 64, (F, 3), generator=g).double() / 16
    d = torch.randint(-16, 16, (F, 3), generator=g).double() / 8
    kind = torch.arange(F) % 3
    fv = torch.randn(F, 3, 3, generator=g).double()
    v1 = torch.where((kind == 0)[:, None], base, base + d)            # kind 0: two coincident corners
    v2 = torch.where((kind == 1)[:, None], base + 2 * d, base - 3 * d)  # kind 1, 2: collinear
    degenerate = torch.stack([base, v1, v2], 1)
    fv[kind < 2] = degenerate[kind < 2]
    fv[kind == 2] = torch.stack([base, base + d, base - 3 * d], 1)[kind == 2]
    fv[::10] = torch.randn(30, 3, 3, generator=g).double()           # some regular faces among them
    deg = torch.ones(F, dtype=torch.bool); deg[::10] = False
    out, fvd, fvr = _fn_case(kal, fv, unit, "degenerate unit=%s" % unit)
    assert torch.equal(out[deg.cuda()], torch.zeros_like(out[deg.cuda()]))
    for sel, what in ((deg, "degenerate"), (~deg, "regular")):
        _gclose(fvd.grad[sel.cuda()], fvr.grad[sel], what="face_normals d/dfv, %s faces" % what)


# ---------------------------------------------------------------------------------------------------------------------
# prepare_vertices and the vertex -> corner CSR
# ---------------------------------------------------------------------------------------------------------------------
def _rotation(rng, n):
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return q


def _fan_mesh(rng, valences, isolated_every=5):
    """fans (hub + ring) with the given hub valences; an isolated vertex after every few fans; faces shuffled and their corners
    rotated, so the vertex lists' corners lie scattered across the face list"""
    verts, faces, isolated = [], [], []
    for i, n in enumerate(valences):
        c = rng.uniform(-0.5, 0.5, 3)
        R = _rotation(rng, 1)[0]
        hub = len(verts)
        verts.append(c)
        closed = i % 2 == 0
        m = n if closed else n + 1
        ang = np.linspace(0, 2 * np.pi * (1 if closed else 0.9), m, endpoint=not closed)
        ring = np.stack([0.3 * np.cos(ang), 0.3 * np.sin(ang), 0.05 * rng.uniform(-1, 1, m)], -1) @ R.T + c
        r0 = len(verts)
        verts.extend(ring)
        for k in range(n):
            faces.append((hub, r0 + k, r0 + (k + 1) % m))
        if i % isolated_every == isolated_every - 1:
            isolated.append(len(verts))
            verts.append(rng.uniform(-0.5, 0.5, 3))
    return np.array(verts), np.array(faces), isolated


def _grid_mesh(nx, ny):
    x, y = np.meshgrid(np.linspace(-0.8, 0.8, nx), np.linspace(-0.8, 0.8, ny), indexing="xy")
    verts = np.stack([x, y, 0.1 * np.sin(3 * x) * np.cos(2 * y)], -1).reshape(-1, 3)
    idx = np.arange(nx * ny).reshape(ny, nx)
    a, b, c, d = idx[:-1, :-1].reshape(-1), idx[:-1, 1:].reshape(-1), idx[1:, :-1].reshape(-1), idx[1:, 1:].reshape(-1)
    faces = np.concatenate([np.stack([a, b, d], -1), np.stack([a, d, c], -1)])
    return verts, faces


def _shuffle_faces(rng, faces):
    faces = faces[rng.permutation(len(faces))]
    cols = (np.arange(3)[None] + rng.integers(0, 3, len(faces))[:, None]) % 3          # each face's corners rotated: same orientation
    return np.take_along_axis(faces, cols, 1)


def _mesh(kind):
    rng = np.random.default_rng({"fans": 1, "grid_and_fans": 2, "grid_12288": 3, "grid_12289": 4}[kind])
    if kind == "fans":                                             # hubs of valence 40, 12 and 13 and longer; V % 32 != 0
        v, f, iso = _fan_mesh(rng, [40, 12, 13, 11, 17, 64, 25, 14, 33, 12, 13, 100])
    elif kind == "grid_and_fans":                                  # long lists scattered over many trips of the builder's threads
        gv, gf = _grid_mesh(40, 50)
        fv_, ff, iso = _fan_mesh(rng, [40, 13, 12, 100, 24, 13, 61, 12, 200, 16], isolated_every=3)
        v = np.concatenate([gv, fv_ * 0.5 + np.array([0.0, 0.0, 0.4])])
        f = np.concatenate([gf, ff + len(gv)])
        iso = [i + len(gv) for i in iso]
    elif kind == "grid_12288":                                     # MM_CSR_MAX_V: the last size the device builder takes
        v, f = _grid_mesh(96, 128); iso = []
    elif kind == "grid_12289":                                     # one isolated vertex more: the host builder
        v, f = _grid_mesh(96, 128)
        v = np.concatenate([v[:5000], [[0.1, 0.2, 0.3]], v[5000:]])
        f = np.where(f >= 5000, f + 1, f); iso = [5000]
    f = _shuffle_faces(rng, f)
    return v.astype(np.float32), f.astype(np.int64), iso


def _camera(rng, B):
    R = _rotation(rng, B)
    T = np.zeros((B, 4, 3))
    T[:, :3] = R
    T[:, 3] = np.array([0.0, 0.0, -3.0]) + rng.uniform(-0.2, 0.2, (B, 3))
    return T.astype(np.float32)


PROJ = np.array([2.5, 2.5, -1.0])


def _prep_ref(v, faces, T, proj):
    """kaolin.render.mesh.prepare_vertices, float64: homogeneous vertices @ transform, perspective_camera, index by faces, unit normals"""
    vc = Fnn.pad(v, (0, 1), value=1.0) @ T
    p = vc * proj.reshape(3)
    vi = p[..., :2] / p[..., 2:3]
    fvc, fvi = vc[:, faces], vi[:, faces]
    return fvc, fvi, _fn_ref(fvc, True)


@pytest.mark.parametrize("kind", ["fans", "grid_and_fans", "grid_12288"])
def test_device_csr_of_synthetic_meshes_is_the_host_builders(kind):
    """lists longer than twelve (the builder's in-place insertion sort), exactly 12 and 13, isolated vertices, V % 32 != 0, and
    V = MM_CSR_MAX_V: offsets and items equal template.vertex_corner_adjacency's, list order included"""
    ops = importlib.import_module("3d-magic-mirror_amd.ops")
    tmpl = importlib.import_module("3d-magic-mirror_amd.template")
    v, f, iso = _mesh(kind)
    V = v.shape[0]
    assert V <= ops._CSR_MAX_V
    faces = torch.from_numpy(f)
    off_h, items_h = tmpl.vertex_corner_adjacency(V, faces)
    val = np.diff(off_h.numpy())
    if kind != "grid_12288":
        assert V % 32 != 0 and val.max() >= 40 and (val == 12).any() and (val == 13).any() and (val[iso] == 0).all()
    for _ in range(2):
        fi, off, items = ops._faces_tables(faces.cuda(), V, DEV)
        assert torch.equal(off.cpu().long(), off_h.long())
        assert torch.equal(items.cpu().long(), items_h.long())
        assert torch.equal(fi.cpu().long(), faces)


@pytest.mark.parametrize("kind,B", [("fans", 1), ("fans", 64), ("grid_and_fans", 3), ("grid_12288", 2), ("grid_12289", 2)])
def test_prepare_vertices_matches_float64(kal, kind, B):
    """values and the gradients to the vertices and to camera_transform against a float64 restatement of kaolin, on both sides of the
    device / host CSR builder switch; isolated vertices get exactly zero gradient; camera_proj on the host and on the device"""
    rng = np.random.default_rng(B)
    v, f, iso = _mesh(kind)
    vb = np.repeat(v[None], B, 0) + rng.normal(size=(B,) + v.shape).astype(np.float32) * 1e-3     # (small: no sliver faces)
    T = _camera(rng, B)
    faces = torch.from_numpy(f)
    ups = [torch.from_numpy(rng.normal(size=s)) for s in ((B, len(f), 3, 3), (B, len(f), 3, 2), (B, len(f), 3))]
    vr, Tr = _ref_leaf(vb), _ref_leaf(T)
    ref = _prep_ref(vr, faces, Tr, torch.from_numpy(PROJ))
    sum(((r * u).sum() for r, u in zip(ref, ups))).backward()
    outs = {}
    for where in ("host", "device"):
        proj = torch.from_numpy(PROJ).float().reshape(3, 1)
        if where == "device":
            proj = proj.cuda()
        vd, Td = _leaf(vb), _leaf(T)
        out = kal.render.mesh.prepare_vertices(vertices=vd, faces=faces, camera_proj=proj, camera_transform=Td)
        for o, r, what in zip(out, ref, ("fvc", "fvi", "fn")):
            _close(o, r, what=what)
        sum(((o * u.float().cuda()).sum() for o, u in zip(out, ups))).backward()
        _gclose(vd.grad, vr.grad, what="d/dvertices")
        _gclose(Td.grad, Tr.grad, what="d/dcamera_transform")
        if iso:
            assert torch.equal(vd.grad[:, iso], torch.zeros_like(vd.grad[:, iso]))
        outs[where] = [o.detach() for o in out] + [vd.grad, Td.grad]
    for a, b in zip(outs["host"], outs["device"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("used", [0, 1, 2])
def test_prepare_vertices_single_outputs_and_a_constant_transform(kal, used):
    """each of the three outputs used alone (the others reach the backward as None), with a camera_transform that does not
    require grad"""
    rng = np.random.default_rng(used)
    B = 3
    v, f, iso = _mesh("fans")
    T = _camera(rng, B)
    faces = torch.from_numpy(f)
    vb = np.repeat(v[None], B, 0)
    vr = _ref_leaf(vb)
    ref = _prep_ref(vr, faces, torch.from_numpy(T).double(), torch.from_numpy(PROJ))[used]
    up = torch.from_numpy(rng.normal(size=ref.shape))
    (ref * up).sum().backward()
    vd, Td = _leaf(vb), _leaf(T, grad=False)
    out = kal.render.mesh.prepare_vertices(vd, faces, torch.from_numpy(PROJ).float().reshape(3, 1).cuda(), camera_transform=Td)[used]
    (out * up.float().cuda()).sum().backward()
    _gclose(vd.grad, vr.grad, what="output %d alone" % used)
    assert Td.grad is None
    assert torch.equal(vd.grad[:, iso], torch.zeros_like(vd.grad[:, iso]))


def test_prepare_vertices_gradients_through_camera_rot_and_trans(kal):
    """camera_rot / camera_trans: (p - t) @ R^T folded into the transform by torch ops, so the gradients reach R and t"""
    rng = np.random.default_rng(2)
    B = 4
    v, f, iso = _mesh("fans")
    faces = torch.from_numpy(f)
    vb = np.repeat(v[None], B, 0)
    R = _rotation(rng, B).astype(np.float32)
    t = (np.array([0.0, 0.0, 3.0]) + rng.uniform(-0.2, 0.2, (B, 3))).astype(np.float32)
    vr, Rr, tr = _ref_leaf(vb), _ref_leaf(R), _ref_leaf(t)
    vc = (vr - tr[:, None]) @ Rr.transpose(1, 2)
    p = vc * torch.from_numpy(PROJ)
    ref = (vc[:, faces], (p[..., :2] / p[..., 2:3])[:, faces])
    ref = ref + (_fn_ref(ref[0], True),)
    ups = [torch.from_numpy(rng.normal(size=r.shape)) for r in ref]
    sum(((r * u).sum() for r, u in zip(ref, ups))).backward()
    vd, Rd, td = _leaf(vb), _leaf(R), _leaf(t)
    out = kal.render.mesh.prepare_vertices(vd, faces, torch.from_numpy(PROJ).float().reshape(3, 1), camera_rot=Rd, camera_trans=td)
    for o, r in zip(out, ref):
        _close(o, r)
    sum(((o * u.float().cuda()).sum() for o, u in zip(out, ups))).backward()
    _gclose(vd.grad, vr.grad, what="d/dvertices")
    _gclose(Rd.grad, Rr.grad, what="d/dcamera_rot")
    _gclose(td.grad, tr.grad, what="d/dcamera_trans")


# ---------------------------------------------------------------------------------------------------------------------
# dibr_rasterization against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _dibr_geometry(oracle, name, B, H, W, seed):
    inp, gt, proj = make_inputs(name, B, H, W, seed=seed)
    T = oracle.camera(inp["distances"], inp["elevations"], inp["azimuths"], inp["biases"])
    fvc, fvi, fn = oracle.prepare_vertices(inp["vertices"], inp["faces"], T, proj)
    return fvc, fvi, fn


def _dibr_case(kal, oracle, B, H, W, D=6, name="sphere", seed=7, kw=None, shift=0.0, backfacing=False, use=("interp", "soft"),
               feat_grad=True, min_cover=0.01):
    kw = dict(kw or {})
    fvc, fvi, fn = _dibr_geometry(oracle, name, B, H, W, seed)
    fvi = (fvi + np.float32(shift)).astype(np.float32)
    fnz = np.full_like(fn[..., 2], -1.0) if backfacing else fn[..., 2]
    rng = np.random.default_rng(seed + D)
    F = fvi.shape[1]
    feats = rng.normal(size=(B, F, 3, D)).astype(np.float32)
    ok = dict(mult=kw.get("multiplier", 1000.0), eps=kw.get("eps", 1e-8))
    sk = dict(sigmainv=kw.get("sigmainv", 7000.0), boxlen=kw.get("boxlen", 0.02), knum=kw.get("knum", 30), mult=ok["mult"])
    valid = (fnz >= 0).astype(np.uint8)
    fidx_o, _, interp_o = oracle.rasterize(H, W, fvc[..., 2], fvi, feats, valid, **ok)
    soft_o, prob, idx, typ = oracle.soft_mask(H, W, fvi, fidx_o, **sk)
    fvid, featd = _leaf(fvi), _leaf(feats, grad=feat_grad)
    interp, soft, fidx = kal.render.mesh.dibr_rasterization(H, W, _leaf(fvc[..., 2], grad=False), fvid, featd, _leaf(fnz, grad=False), **kw)
    assert interp.shape == (B, H, W, D) and soft.shape == (B, H, W) and fidx.shape == (B, H, W)
    assert np.array_equal(fidx.cpu().numpy(), fidx_o), int((fidx.cpu().numpy() != fidx_o).sum())
    if backfacing:
        assert (fidx_o == -1).all()
    else:
        assert (fidx_o >= 0).mean() > min_cover
    _close(interp, interp_o, 1e-5, "interp")
    _close(soft, soft_o, 1e-4, "soft")
    assert ((soft_o > 0.01) & (soft_o < 0.99)).mean() > 0.001
    g_i = rng.normal(size=interp_o.shape).astype(np.float32)
    g_s = rng.normal(size=soft_o.shape).astype(np.float32)
    loss = 0
    if "interp" in use:
        loss = loss + (interp * _leaf(g_i, grad=False)).sum()
    if "soft" in use:
        loss = loss + (soft * _leaf(g_s, grad=False)).sum()
    loss.backward()

    def refs(dtype):
        dfvi = np.zeros(fvi.shape, dtype); dfeat = np.zeros(feats.shape, dtype)
        if "interp" in use:
            a, b = oracle.rasterize_backward(g_i, fidx_o, fvi, feats, dtype=dtype, **ok)
            dfvi = dfvi + a; dfeat = dfeat + b
        if "soft" in use:
            if dtype == np.float32:
                p, i, t = prob, idx, typ
            else:
                _, p, i, t = oracle.soft_mask(H, W, fvi, fidx_o, dtype=dtype, **sk)
            dfvi = dfvi + oracle.soft_mask_backward(g_s, fidx_o, fvi, p, i, t, sigmainv=sk["sigmainv"], mult=sk["mult"], dtype=dtype)
        return dfvi, dfeat

    dfvi_o, dfeat_o = refs(np.float32)
    _gclose(fvid.grad, dfvi_o, what="dibr d/dfvi", ref64=lambda: refs(np.float64)[0])
    if feat_grad:
        _gclose(featd.grad, dfeat_o, what="dibr d/dfeatures", ref64=lambda: refs(np.float64)[1])
    else:
        assert featd.grad is None
    return fidx_o, soft_o


@pytest.mark.parametrize("H,W", [(128, 64), (64, 128), (50, 94)])
def test_dibr_rasterization_non_square_screens(kal, oracle, H, W):
    _dibr_case(kal, oracle, 2, H, W)


@pytest.mark.parametrize("S,B", [(256, 2), (272, 2), (1040, 1)])
def test_dibr_rasterization_order_launch_thresholds(kal, oracle, S, B):
    """1024 tile slots (no bin-count pre-pass), 1156 (with it), and 16900 > MM_ORDER_MAX_SLOTS: no launch order, the walk runs in
    natural order in block mode"""
    _dibr_case(kal, oracle, B, S, S, min_cover=0.005)


@pytest.mark.parametrize("D", [1, 8, 9, 32])
def test_dibr_rasterization_feature_channels(kal, oracle, D):
    """up to 8 channels the backward adds in registers; more take the per-face LDS accumulators (float atomics)"""
    _dibr_case(kal, oracle, 3, 64, 48, D=D, name="smpl_uv_642")


def test_dibr_rasterization_more_than_32_channels_raise(kal, oracle):
    fvc, fvi, fn = _dibr_geometry(oracle, "sphere", 1, 32, 32, 7)
    with pytest.raises(RuntimeError):
        kal.render.mesh.dibr_rasterization(32, 32, _leaf(fvc[..., 2]), _leaf(fvi), torch.zeros(1, fvi.shape[1], 3, 33, device=DEV),
                                           _leaf(fn[..., 2]))


def test_dibr_rasterization_multiplier_and_eps_away_from_defaults(kal, oracle):
    _dibr_case(kal, oracle, 2, 80, 72, kw=dict(multiplier=640.0, eps=1e-5, sigmainv=5000.0, boxlen=0.03, knum=12))


@pytest.mark.parametrize("use,feat_grad", [(("interp",), True), (("interp", "soft"), False), (("soft",), False)])
def test_dibr_rasterization_partial_backwards(kal, oracle, use, feat_grad):
    """interp-only backward (no soft-mask gradient); features that do not require grad"""
    _dibr_case(kal, oracle, 2, 64, 64, use=use, feat_grad=feat_grad)


def test_dibr_rasterization_every_face_back_facing(kal, oracle):
    """nothing is rasterised (face_idx all -1, interpolated features all zero) but the soft mask is still built from every face"""
    fidx_o, soft_o = _dibr_case(kal, oracle, 2, 64, 64, backfacing=True)
    assert soft_o.max() > 0.5


def test_dibr_rasterization_mesh_partly_off_screen(kal, oracle):
    fidx_o, soft_o = _dibr_case(kal, oracle, 2, 64, 80, shift=0.75)
    assert (fidx_o[..., -1] >= 0).any() and (fidx_o[..., 0] < 0).all()


def test_diff_render_beyond_the_order_launchs_slots_matches_oracle(pkg, oracle):
    """DiffRender.render + recon_data + backward on a 1040x1040 screen (16 900 tile slots: no launch order, natural-order walk in
    block mode in the fused kernels) against the oracle, as tests/test_gpu_parity.py does at smaller screens"""
    B, S = 1, 1040
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), S, emit_imnormal=True)
    H, W = dr.render_height, dr.image_size
    att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, B, H, W, seed=3)
    datt = {k: (v.to(DEV).requires_grad_(k in LEAVES) if torch.is_tensor(v) else v) for k, v in att.items()}
    inp = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in att.items()}
    inp["faces"] = dr.faces.numpy().astype(np.int32)
    inp["face_uvs"] = dr.face_uvs.numpy()[0]
    proj = dr.cam_proj.numpy().reshape(3)
    rgbs, out = dr.render(no_mask=True, **datt)
    wfn = torch.from_numpy(np.random.default_rng(3).normal(size=(B, dr.num_faces, 3)).astype(np.float32) * 1e-3)
    loss = dr.recon_data(rgbs, gt.to(DEV), no_mask=True) + (out["face_normals"] * wfn.to(DEV)).sum()
    loss.backward()
    rgba_o, fidx_o, fn_o, imn_o = oracle.render_forward(inp, H, W, True, proj)
    loss_o, dpred = oracle.recon_data(rgba_o.transpose(0, 3, 1, 2), gt.numpy(), image_weight=dr.image_weight, want_grad=True)
    g_o = oracle.render_backward(inp, H, W, True, proj, np.ascontiguousarray(dpred.transpose(0, 2, 3, 1)), wfn.numpy())
    fidx = dr.last_face_idx.cpu().numpy()
    assert (fidx == fidx_o).all(), "face_idx mismatches: %d" % int((fidx != fidx_o).sum())
    assert (fidx >= 0).mean() > 0.005
    _close(rgbs.detach().permute(0, 2, 3, 1), rgba_o)
    _close(out["imnormal"], imn_o, 1e-6)
    assert abs(float(loss.detach()) - (loss_o + float((fn_o * wfn.numpy()).sum()))) < 2e-5
    for k in LEAVES:
        assert np.abs(g_o[k]).max() > 0, k
        _gclose(datt[k].grad, g_o[k], what=k)
