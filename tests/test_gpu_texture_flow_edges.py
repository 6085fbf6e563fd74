"""Texture-flow sampling (csrc/mm_texflow.hip) at the shapes, flows and input types its ordinary test never reaches.

Reference: the float64 CPU evaluation of tests/test_gpu_texture_flow.py::_reference (ATen's bicubic grid_sample, align_corners=True,
zeros padding, then the vertical mirror).  Bars, from that module: output 2e-5 absolute, gradients 1e-4 * max(1, max|ref|).
Every case id names the branch or loop bound of the kernel it is built to reach; where a branch is selected by a structural
precondition (W < 4, t == 0, all taps outside, the window shift, the saturating guard) the test asserts that precondition on its
own inputs, evaluated in float32 exactly as the kernel evaluates it, before it looks at any output.

Half and bfloat16 inputs: the reference is float64 on the values AFTER rounding to that type.  The output of the kernel is
float32 and holds the ordinary bar.  A gradient with respect to a half / bfloat16 tensor is, by autograd's contract, a tensor of
that type: the kernel's float32 gradient is rounded once to it.  That one rounding is allowed for on top of the ordinary bar,
element by element, as u * |ref| with u the unit roundoff of the format (2^-11 for half, 2^-8 for bfloat16) -- a property of the
number format, not of the kernel.

The image gradient uses float atomics and is exempt from bitwise run-to-run equality (tests/test_gpu_float_atomics.py owns its
spread); it holds the ordinary gradient bar here, also where thousands of adds land on one texel.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT_BAR = 2e-5
GRAD_BAR = 1e-4
UNIT_ROUNDOFF = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def _reference(img, flow):
    t = F.grid_sample(img, flow.permute(0, 2, 3, 1), mode='bicubic', align_corners=True)
    return torch.cat([t, t.flip([2])], dim=2)


def _kernel_coords(flow, H, W):
    """ix, iy as the kernel forms them: float32, ((g + 1) / 2) * (size - 1)."""
    f = flow.to(torch.float32)
    one, two = torch.tensor(1.0, dtype=torch.float32), torch.tensor(2.0, dtype=torch.float32)
    ix = ((f[:, 0] + one) / two) * torch.tensor(float(W - 1), dtype=torch.float32)
    iy = ((f[:, 1] + one) / two) * torch.tensor(float(H - 1), dtype=torch.float32)
    return ix, iy


def _smooth_flow(B, Ho, Wo, spread, noise, g):
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, Ho), torch.linspace(-1, 1, Wo), indexing="ij")
    return (torch.stack([xs, ys], 0)[None] * spread + noise * torch.randn(B, 2, Ho, Wo, generator=g)).contiguous()


def _check(pkg, img, flow, wgt, tag, dev_img=None, dev_flow=None, want_image_grad=True):
    """Forward and both gradients of sample_texture against the float64 reference on the same (already rounded) values.

    img / flow: CPU tensors of any float type (the reference reads them as float64).  dev_img / dev_flow: optional device tensors to
    hand to the kernel instead of plain copies (non-contiguous views).  Non-finite reference texels: the output must be NaN exactly
    there; their upstream gradient is zeroed; the flow gradient at those texels themselves is not compared (ATen gives NaN, the
    kernel's masking gives 0; either is acceptable)."""
    B, C, H, W = img.shape
    Ho, Wo = flow.shape[2:]
    img_h, flow_h = img.double().requires_grad_(True), flow.double().requires_grad_(True)
    ref = _reference(img_h, flow_h)
    bad = ~torch.isfinite(ref.detach())
    wgt = wgt.clone()
    wgt[bad] = 0.0
    (torch.where(bad, torch.zeros_like(ref), ref) * wgt.double()).sum().backward()

    img_d = (img.to(DEV) if dev_img is None else dev_img).detach().requires_grad_(want_image_grad)
    flow_d = (flow.to(DEV) if dev_flow is None else dev_flow).detach().requires_grad_(True)
    out = pkg.sample_texture(img_d, flow_d)
    assert out.shape == (B, C, 2 * Ho, Wo) and out.dtype == torch.float32
    out_c = out.detach().cpu()
    assert torch.equal(torch.isnan(out_c), bad), tag + ": NaN exactly where the reference has it"
    assert bool((torch.isnan(ref.detach()) == bad).all()), tag + ": the reference's non-finite texels are NaN, not inf"
    front, back = out_c[:, :, :Ho], out_c[:, :, Ho:].flip([2])
    assert torch.equal(torch.nan_to_num(front, nan=7.0), torch.nan_to_num(back, nan=7.0)), tag + ": back == mirrored front, exactly"
    (torch.where(bad.to(DEV), torch.zeros_like(out), out) * wgt.to(DEV)).sum().backward()

    err = float((out_c.double() - ref.detach())[~bad].abs().max()) if bool((~bad).any()) else 0.0
    print("%s: output err %.3e (bar %.1e)" % (tag, err, OUT_BAR))
    assert err <= OUT_BAR, (tag, "output", err)

    flow_bad = (bad[:, :, :Ho] | bad[:, :, Ho:].flip([2])).any(1, keepdim=True).expand(B, 2, Ho, Wo) | ~torch.isfinite(flow.double())
    pairs = [(flow_d.grad, flow_h.grad, "flow", flow_bad, flow.dtype)]
    if want_image_grad:
        pairs.append((img_d.grad, img_h.grad, "image", torch.zeros_like(img_h.grad, dtype=torch.bool), img.dtype))
    for got, want, nm, skip, dt in pairs:
        assert got is not None and got.shape == want.shape, (tag, nm)
        got = got.cpu().double()
        assert bool(torch.isfinite(got[~skip]).all()) and bool(torch.isfinite(want[~skip]).all()), (tag, nm, "finite where compared")
        scale = max(1.0, float(want[~skip].abs().max())) if bool((~skip).any()) else 1.0
        allowed = GRAD_BAR * scale + UNIT_ROUNDOFF[dt] * want.abs()
        excess = ((got - want).abs() - allowed)[~skip]
        err = float((got - want).abs()[~skip].max()) if bool((~skip).any()) else 0.0
        print("%s: d/d%s err %.3e (bar %.1e * %.3g)" % (tag, nm, err, GRAD_BAR, scale))
        assert float(excess.max()) <= 0.0 if excess.numel() else True, (tag, nm, err, scale)
    return out_c, flow_d.grad.cpu(), ref.detach(), flow_h.grad


# ---------------------------------------------------------------------------------------------------------------------------------
# load_row's narrow branch (W < 4: four scalar loads through the clamped xs[]) and the zero coordinate scale of W == 1 / H == 1
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [
    pytest.param(6, 3, id="W3-narrow-row-scalar-loads"),
    pytest.param(6, 2, id="W2-narrow-row-scalar-loads"),
    pytest.param(5, 1, id="W1-narrow-row-zero-x-scale"),
    pytest.param(1, 7, id="H1-zero-y-scale-wide-row"),
    pytest.param(1, 3, id="H1-W3-zero-y-scale-narrow-row"),
    pytest.param(1, 1, id="H1-W1-single-texel-image"),
])
def test_texture_flow_narrow_images(pkg, H, W):
    """Rows narrower than four texels take load_row's `else` branch; (W-1)/2 == 0 or (H-1)/2 == 0 zeroes that flow gradient."""
    narrow_rows = W < 4
    assert narrow_rows or H == 1                                 # the precondition that routes execution to the branch named in the id
    g = torch.Generator().manual_seed(100 + 10 * H + W)
    B, C, Ho, Wo = 2, 3, 7, 70
    img = torch.rand(B, C, H, W, generator=g)
    flow = _smooth_flow(B, Ho, Wo, 1.2, 0.2, g)
    wgt = torch.randn(B, C, 2 * Ho, Wo, generator=g)
    _, gflow, _, gflow_ref = _check(pkg, img, flow, wgt, "narrow H%d W%d" % (H, W))
    if W == 1:
        assert float(gflow[:, 0].abs().max()) == 0.0 and float(gflow_ref[:, 0].abs().max()) == 0.0
    if H == 1:
        assert float(gflow[:, 1].abs().max()) == 0.0 and float(gflow_ref[:, 1].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# flow exactly on texel centres (t == 0), exactly on the border, one ulp outside it
# ---------------------------------------------------------------------------------------------------------------------------------
def test_texture_flow_exact_texel_centres_and_borders(pkg):
    """t == 0: W - 1 and H - 1 are powers of two, so -1 + 2 i / (W - 1) is exact in float32 and the kernel's ix is the integer i.
    The flow gradient is continuous there (the cubic kernel is C1): no texel is excluded from the comparison."""
    B, C, H, W = 2, 3, 5, 9
    g = torch.Generator().manual_seed(7)
    img = torch.rand(B, C, H, W, generator=g)
    xs = -1.0 + 2.0 * torch.arange(W, dtype=torch.float32) / (W - 1)
    ys = -1.0 + 2.0 * torch.arange(H, dtype=torch.float32) / (H - 1)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    flow = torch.stack([gx, gy], 0)[None].repeat(B, 1, 1, 1).contiguous()
    # image 1: centres in x only, y in between; plus the four corners are exactly (-1 / +1, -1 / +1) in both images
    flow[1, 1] += 0.3 * torch.rand(H, W, generator=g) / (H - 1)
    ix, iy = _kernel_coords(flow, H, W)
    assert torch.equal(ix, ix.floor()) and torch.equal(iy[0], iy[0].floor())          # t == 0 in the kernel's own arithmetic
    assert float(flow[0, 0].min()) == -1.0 and float(flow[0, 0].max()) == 1.0 and float(flow[0, 1].min()) == -1.0 and float(flow[0, 1].max()) == 1.0
    wgt = torch.randn(B, C, 2 * H, W, generator=g)
    out, _, _, _ = _check(pkg, img, flow, wgt, "texel centres")
    # at t == 0 the cubic weights are (0, 1, 0, 0): the sample IS the texel, to the bit
    assert torch.equal(out[0, :, :H], img[0])


def test_texture_flow_one_ulp_outside_the_border(pkg):
    """Flow at nextafter(+-1, +-2) and nextafter(+-1, 0): the coordinate sits on, or one rounding off, the last texel centre."""
    B, C, H, W = 1, 3, 6, 8
    g = torch.Generator().manual_seed(8)
    img = torch.rand(B, C, H, W, generator=g)
    one = np.float32(1.0)
    edge = torch.tensor([np.nextafter(one, np.float32(2)), one, np.nextafter(one, np.float32(0)),
                         -np.nextafter(one, np.float32(2)), -one, -np.nextafter(one, np.float32(0))], dtype=torch.float32)
    n = edge.numel()
    assert float(edge[0]) > 1.0 and float(edge[3]) < -1.0
    gy, gx = torch.meshgrid(edge, edge, indexing="ij")
    flow = torch.stack([gx, gy], 0)[None].contiguous()
    wgt = torch.randn(B, C, 2 * n, n, generator=g)
    _check(pkg, img, flow, wgt, "one ulp outside")


# ---------------------------------------------------------------------------------------------------------------------------------
# all sixteen taps outside the image
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [pytest.param(9, id="all-taps-outside-wide-row"), pytest.param(3, id="all-taps-outside-narrow-row")])
def test_texture_flow_all_taps_outside(pkg, W):
    B, C, H = 2, 3, 6
    g = torch.Generator().manual_seed(9 + W)
    img = 0.25 + torch.rand(B, C, H, W, generator=g)
    # W == 3: a flow of -3 puts ix on -2, whose last tap is texel 0 (with weight 0): one step further out leaves no tap inside
    vals = torch.tensor([3.0, -3.0, 1e30, -1e30, 4.5, -4.5] if W == 9 else [4.0, -4.0, 1e30, -1e30, 5.5, -5.5], dtype=torch.float32)
    Ho, Wo = 4, vals.numel() * 2
    flow = _smooth_flow(B, Ho, Wo, 0.8, 0.1, g)
    flow[:, 0, :, :vals.numel()] = vals                          # x far outside, y inside
    flow[:, 1, :, vals.numel():] = vals                          # y far outside, x inside
    ix, iy = _kernel_coords(flow, H, W)
    x0, y0 = ix.floor() - 1, iy.floor() - 1
    outside = (x0 >= W) | (x0 + 3 < 0) | (y0 >= H) | (y0 + 3 < 0)
    assert bool(outside.all())                                   # no tap of any texel is inside the image
    wgt = torch.randn(B, C, 2 * Ho, Wo, generator=g)
    out, gflow, ref, gflow_ref = _check(pkg, img, flow, wgt, "all taps outside W%d" % W)
    assert float(ref.abs().max()) == 0.0 and float(gflow_ref.abs().max()) == 0.0
    assert float(out.abs().max()) == 0.0 and float(gflow.abs().max()) == 0.0          # exactly 0, sign included in the comparison above


# ---------------------------------------------------------------------------------------------------------------------------------
# the 16-byte row load's window shift: x0 = -3, -2, -1 (sh < 0, k <= 0) and x0 = W-3, W-2, W-1 (sh > 0, k >= 3)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x0_of", [
    pytest.param(lambda W: -3, id="x0=-3-window-shift-sh-3-one-tap-inside"),
    pytest.param(lambda W: -2, id="x0=-2-window-shift-sh-2"),
    pytest.param(lambda W: -1, id="x0=-1-window-shift-sh-1"),
    pytest.param(lambda W: 0, id="x0=0-window-unshifted-left"),
    pytest.param(lambda W: W - 4, id="x0=W-4-window-unshifted-right"),
    pytest.param(lambda W: W - 3, id="x0=W-3-window-shift-sh+1"),
    pytest.param(lambda W: W - 2, id="x0=W-2-window-shift-sh+2"),
    pytest.param(lambda W: W - 1, id="x0=W-1-window-shift-sh+3-one-tap-inside"),
])
@pytest.mark.parametrize("W", [pytest.param(9, id="W9"), pytest.param(4, id="W4-window-is-the-row")])
def test_texture_flow_row_window_shift(pkg, W, x0_of):
    """Every texel of the case has the same, deliberate x0; fractions and rows vary.  The image is a ramp plus noise, so that a tap
    read from the wrong window slot changes the sample by far more than the bar."""
    x0 = x0_of(W)
    B, C, H, Ho, Wo = 2, 3, 6, 5, 24
    g = torch.Generator().manual_seed(1000 + 10 * W + (x0 + 5))
    img = (torch.arange(W, dtype=torch.float32)[None, None, None] * 0.5 + torch.rand(B, C, H, W, generator=g)).contiguous()
    frac = 0.05 + 0.9 * torch.rand(B, Ho, Wo, generator=g)
    if W == 9:
        frac[:, :, 0] = 0.0                                      # and one column exactly on the texel centre (W - 1 a power of two: exact)
    flow = _smooth_flow(B, Ho, Wo, 0.9, 0.1, g)
    flow[:, 0] = ((x0 + 1) + frac) * 2.0 / (W - 1) - 1.0
    ix, _ = _kernel_coords(flow, H, W)
    assert bool((ix.floor() - 1 == x0).all())                    # the kernel's own float32 arithmetic lands every texel on this x0
    xw = min(max(x0, 0), W - 4)
    assert (x0 - xw != 0) == (x0 < 0 or x0 > W - 4)              # sh != 0 exactly for the shifted ids
    wgt = torch.randn(B, C, 2 * Ho, Wo, generator=g)
    _check(pkg, img, flow, wgt, "x0=%d W=%d" % (x0, W))


# ---------------------------------------------------------------------------------------------------------------------------------
# the saturating float -> int guard: |floor(ix)| > 2e9, +-inf, NaN
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [pytest.param(9, id="saturating-guard-wide-row"), pytest.param(2, id="saturating-guard-narrow-row"),
                               pytest.param(1, id="saturating-guard-W1-inf-times-zero")])
def test_texture_flow_huge_and_non_finite_flow(pkg, W):
    """|fx| > 2e9 (beyond int32, where a plain cast is undefined), +-1e30, +-inf and NaN.  ATen samples 0 with zero flow gradient for
    the finite ones and NaN for inf / NaN; the image gradient stays finite once the NaN texels get zero upstream gradient."""
    B, C, H = 2, 3, 5
    g = torch.Generator().manual_seed(50 + W)
    img = 0.25 + torch.rand(B, C, H, W, generator=g)
    inf, nan = float("inf"), float("nan")
    vals = torch.tensor([1e9, -1e9, 3e9, -3e9, 1e10, -1e10, 1e30, -1e30, inf, -inf, nan], dtype=torch.float32)
    sure = torch.nonzero(~(vals.abs() < 1e10)).reshape(-1)        # |floor(coordinate)| > 2e9 for every image size of this test, or non-finite
    n = vals.numel()
    Ho, Wo = 3, 2 * n + 6
    flow = _smooth_flow(B, Ho, Wo, 0.8, 0.1, g)
    flow[:, 0, :, :n] = vals
    flow[:, 1, :, n:2 * n] = vals
    flow[1, 1, :, :n] = vals.flip(0)                             # both coordinates wild in image 1
    ix, iy = _kernel_coords(flow, H, W)
    fx, fy = ix.floor(), iy.floor()
    guard = ~((fx >= -2e9) & (fx <= 2e9)) | ~((fy >= -2e9) & (fy <= 2e9))
    assert bool(guard[:, :, n + sure].all())                     # y: these columns take the guard's INT_MIN / 2 side ...
    if W > 1:
        assert bool(guard[:, :, sure].all())                     # ... and so do they in x
    else:
        assert bool(torch.isnan(ix[:, :, n - 3:n]).all()) and bool((ix[:, :, :n - 3] == 0).all())     # x: finite * 0 == 0 is tame, inf * 0 is NaN
    tame = ~guard[:, :, :2 * n]                                  # 1e9 and 3e9 on a small image: beyond int32 for some sizes, castable for others
    assert bool(((fx.abs() >= 4e8) | (fy.abs() >= 4e8) | (W == 1))[:, :, :2 * n][tame].all())
    assert not bool(guard[:, :, 2 * n:].any())                   # and the rest of the row is ordinary
    wgt = torch.randn(B, C, 2 * Ho, Wo, generator=g)
    out, gflow, ref, _ = _check(pkg, img, flow, wgt, "wild flow W%d" % W)
    assert bool(torch.isnan(ref).any()) and bool((ref == 0).any())
    finite_wild = guard & torch.isfinite(flow[:, 0]) & torch.isfinite(flow[:, 1])
    assert bool(finite_wild.any())
    m = finite_wild[:, None].expand(B, 2, Ho, Wo)
    assert float(gflow[m].abs().max()) == 0.0                    # huge but finite: sample 0, gradient 0, exactly
    assert float(out[:, :, :Ho][finite_wild[:, None].expand(B, C, Ho, Wo)].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# C == 1, non-contiguous inputs, half and bfloat16 inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_texture_flow_single_channel(pkg):
    B, C, H, W, Ho, Wo = 3, 1, 11, 13, 9, 66
    g = torch.Generator().manual_seed(21)
    img = torch.rand(B, C, H, W, generator=g)
    flow = _smooth_flow(B, Ho, Wo, 1.1, 0.15, g)
    _check(pkg, img, flow, torch.randn(B, C, 2 * Ho, Wo, generator=g), "C == 1")


@pytest.mark.parametrize("which", [pytest.param("image", id="non-contiguous-image-channel-slice-and-transpose"),
                                   pytest.param("flow", id="non-contiguous-flow-channels-last-decoder-output"),
                                   pytest.param("both", id="non-contiguous-both-strided-columns")])
def test_texture_flow_non_contiguous_inputs(pkg, which):
    B, C, H, W, Ho, Wo = 2, 3, 10, 12, 8, 40
    g = torch.Generator().manual_seed(22)
    img = torch.rand(B, C, H, W, generator=g)
    flow = _smooth_flow(B, Ho, Wo, 1.1, 0.15, g)
    dev_img, dev_flow = None, None
    if which in ("image", "both"):
        big = torch.zeros(B, C + 2, W, H + 1, device=DEV)        # channel slice of a larger tensor, rows / columns transposed
        big[:, 1:1 + C, :, :H] = img.to(DEV).transpose(2, 3)
        dev_img = big[:, 1:1 + C, :, :H].transpose(2, 3)
        assert not dev_img.is_contiguous() and torch.equal(dev_img.cpu(), img)
    if which == "flow":
        dev_flow = flow.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)       # (B,Ho,Wo,2) memory seen as (B,2,Ho,Wo)
        assert not dev_flow.is_contiguous() and torch.equal(dev_flow.cpu(), flow)
    if which == "both":
        wide = torch.zeros(B, 2, Ho, 2 * Wo, device=DEV)
        wide[:, :, :, ::2] = flow.to(DEV)
        dev_flow = wide[:, :, :, ::2]
        assert not dev_flow.is_contiguous() and torch.equal(dev_flow.cpu(), flow)
    _check(pkg, img, flow, torch.randn(B, C, 2 * Ho, Wo, generator=g), "non-contiguous " + which, dev_img=dev_img, dev_flow=dev_flow)


@pytest.mark.parametrize("dtype,which", [
    pytest.param(torch.float16, "image", id="half-image-float32-flow"),
    pytest.param(torch.float16, "both", id="half-image-half-flow"),
    pytest.param(torch.bfloat16, "image", id="bfloat16-image-float32-flow"),
    pytest.param(torch.bfloat16, "both", id="bfloat16-image-bfloat16-flow"),
])
def test_texture_flow_reduced_precision_inputs(pkg, dtype, which):
    """The wrapper widens half / bfloat16 inputs to float32: the reference is float64 on the values after rounding to that type, the
    float32 output holds the ordinary bar, and the gradients come back in the inputs' own types (module docstring)."""
    B, C, H, W, Ho, Wo = 2, 3, 12, 10, 9, 33
    g = torch.Generator().manual_seed(23)
    img = torch.rand(B, C, H, W, generator=g).to(dtype)
    flow = _smooth_flow(B, Ho, Wo, 1.1, 0.15, g)
    if which == "both":
        flow = flow.to(dtype)
    _check(pkg, img, flow, torch.randn(B, C, 2 * Ho, Wo, generator=g), "%s %s" % (dtype, which))


# ---------------------------------------------------------------------------------------------------------------------------------
# image gradient: thousands of float atomic adds on the same source texel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centre", [pytest.param(False, id="constant-flow-16-texels-take-every-atomic-add"),
                                    pytest.param(True, id="constant-flow-on-a-texel-centre-one-texel-takes-them-all")])
def test_texture_flow_image_gradient_under_contention(pkg, centre):
    """Constant flow: all Ho * Wo = 4096 sampled texels (x 2 mirrored rows, folded in registers) scatter to the same 4 x 4 source
    texels of their image, 4096 atomic adds each.  Held to the ordinary gradient bar against float64."""
    B, C, H, W, Ho, Wo = 2, 3, 17, 17, 64, 64
    g = torch.Generator().manual_seed(31)
    img = torch.rand(B, C, H, W, generator=g)
    flow = torch.empty(B, 2, Ho, Wo)
    if centre:
        flow[:, 0], flow[:, 1] = -1.0 + 2.0 * 5 / (W - 1), -1.0 + 2.0 * 11 / (H - 1)          # exact: W - 1 == H - 1 == 16
        ix, iy = _kernel_coords(flow, H, W)
        assert bool((ix == 5).all()) and bool((iy == 11).all())
    else:
        flow[:, 0], flow[:, 1] = 0.2371, -0.4113
    assert bool((flow == flow[:, :, :1, :1]).all())
    wgt = torch.randn(B, C, 2 * Ho, Wo, generator=g)
    img_h = img.double().requires_grad_(True)
    (_reference(img_h, flow.double()) * wgt.double()).sum().backward()
    hit = int((img_h.grad[0, 0] != 0).sum())
    assert hit == (1 if centre else 16)                          # every add of an image plane lands on these few texels
    _check(pkg, img, flow, wgt, "contended image gradient")
