"""Template-anchored encoder features on the MI355X (csrc/mm_encfeat.hip) against the reference formula restated in float64 on the
host (tests/test_encoder_features_host.py: shape_ref / camera_ref).  Bars: forward max|got - ref| <= 1e-5 max|ref|; every gradient
within 1e-4 of its own maximum (tests/parity_bar.py rel_errors)."""
import importlib

import pytest
import torch

from parity_bar import rel_errors
from test_encoder_features_host import camera_ref, shape_ref, template_lpl

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EF = importlib.import_module("3d-magic-mirror_amd.encoder_features")
FWD_BAR, GRAD_BAR = 1e-5, 1e-4


def _close(got, ref, bar, what):
    e, _ = rel_errors(got.detach().double().cpu(), ref.detach().double().cpu())
    assert e <= bar, (what, e)


def _run(op, x, template, params, g, extra=()):
    """ours: (out, grad x, grads of params) on the device"""
    xd = x.to(DEV).requires_grad_()
    pd = [q.to(DEV).requires_grad_() for q in params]
    if op == "shape":
        out = EF.shape_features(xd, template.to(DEV), extra[0], pd[0])
    else:
        out = EF.camera_features(xd, template.to(DEV), pd[0], pd[1])
    out.backward(g.to(DEV))
    return out, xd.grad, [q.grad for q in pd]


def _reference(op, x, template, params, g, extra=()):
    x64 = x.double().requires_grad_()
    p64 = [q.double().requires_grad_() for q in params]
    ref = shape_ref(x64, template, extra[0].cpu(), p64[0]) if op == "shape" else camera_ref(x64, template, p64[0], p64[1])
    ref.backward(g.double())
    return ref, x64.grad, [q.grad for q in p64]


def check(op, x, template, params, lpl=None, seed=0, grad_bar=GRAD_BAR):
    extra = (lpl,) if op == "shape" else ()
    B, C = x.shape[:2]
    V = template.shape[-2]
    shape = (B, 3 * C + 3, V) if op == "shape" else (B, 2 * C, 2, 2)
    g = torch.randn(shape, generator=torch.Generator().manual_seed(seed + 1))
    out, gx, gp = _run(op, x, template, params, g, extra)
    ref, rgx, rgp = _reference(op, x, template, params, g, extra)
    assert out.dtype == torch.float32 and out.shape == ref.shape
    assert gx.dtype == x.dtype and gx.shape == x.shape
    _close(out, ref, FWD_BAR, "forward")
    _close(gx.float(), rgx, grad_bar, "grad x")
    for i, (a, b) in enumerate(zip(gp, rgp)):
        _close(a, b, GRAD_BAR, "grad p%d" % i)
    return out, gx, gp


def rand_x(B, C, H, W, seed=0):
    return torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed))


# ---- the benchmark shapes (tools/bench_encoder_features.py), the templates' own Laplacians ---------------------------------------
# The op is run on the whole batch; planes are independent, so the float64 reference is formed for a slice of the channels (the
# gradient of p, a sum over every plane, is formed in closed form over all of them).
BENCH = [(32, 2048, 4, 4, "sphere"), (48, 288, 8, 8, "sphere"), (32, 2048, 4, 2, "sphere"), (32, 2048, 4, 4, "smpl_uv")]


@pytest.mark.parametrize("B,C,H,W,tname", BENCH)
def test_benchmark_shapes(B, C, H, W, tname):
    template, lpl = template_lpl(tname)
    V = template.shape[1]
    x = rand_x(B, C, H, W, seed=B + C)
    sel = torch.arange(0, C, max(C // 24, 1))[:24]
    gen = torch.Generator().manual_seed(5)
    p, pm, pl = torch.tensor([0.3]), torch.tensor([-0.7]), torch.tensor([1.1])
    # shape
    gs = torch.randn(B, 3 * C + 3, V, generator=gen)
    out, gx, gp = _run("shape", x, template, [p], gs, (lpl.to(DEV),))
    rows = torch.cat((sel, C + sel, 2 * C + sel, torch.arange(3 * C, 3 * C + 3)))
    g_sub = torch.cat((gs[:, sel], gs[:, C + sel], gs[:, 2 * C + sel], gs[:, 3 * C:]), 1)
    xs = x[:, sel].double().requires_grad_()
    ref = shape_ref(xs, template, lpl, p.double())
    ref.backward(g_sub.double())
    _close(out[:, rows], ref, FWD_BAR, "shape forward")
    _close(gx[:, sel].float(), xs.grad, GRAD_BAR, "shape grad x")
    x64, w = x.double(), torch.sigmoid(p.double())
    mx, mean = x64.flatten(2).max(-1).values, x64.flatten(2).mean(-1)
    dp = (gs[:, C:2 * C].double().sum(-1) * (mx - mean)).sum() * w * (1 - w)
    _close(gp[0], dp, GRAD_BAR, "shape grad p")
    del out, gx
    # camera
    gc = torch.randn(B, 2 * C, 2, 2, generator=gen)
    out, gx, (gpm, gpl) = _run("camera", x, template, [pm, pl], gc)
    xs = x[:, sel].double().requires_grad_()
    ref = camera_ref(xs, template, pm.double(), pl.double())
    ref.backward(torch.cat((gc[:, sel], gc[:, C + sel]), 1).double())
    _close(out[:, torch.cat((sel, C + sel))], ref, FWD_BAR, "camera forward")
    _close(gx[:, sel].float(), xs.grad, GRAD_BAR, "camera grad x")
    with torch.no_grad():                                              # the p gradients over every plane, in float64 on the device
        xd = x.to(DEV).double()
        pooled = [torch.nn.functional.adaptive_max_pool2d(xd, 2) - torch.nn.functional.adaptive_avg_pool2d(xd, 2)]
        uv = template.to(DEV).double().reshape(1, V, 1, 3)[..., :2].repeat(B, 1, 1, 1)
        loc = torch.nn.functional.grid_sample(xd, uv, mode="bilinear", align_corners=False)
        pooled.append(torch.nn.functional.adaptive_max_pool2d(loc, 2) - torch.nn.functional.adaptive_avg_pool2d(loc, 2))
        for got, q, half, d in ((gpm, pm, 0, pooled[0]), (gpl, pl, 1, pooled[1])):
            wq = torch.sigmoid(q.double()).to(DEV)
            ref_p = (gc[:, half * C:(half + 1) * C].to(DEV).double() * d).sum() * wq * (1 - wq)
            _close(got, ref_p.cpu(), GRAD_BAR, "camera grad p%d" % half)


# ---- the semantics at the edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pval", [-3.0, 0.0, 2.5])
def test_ragged_sphere2(pval):
    template, lpl = template_lpl("sphere2")
    x = rand_x(3, 37, 5, 7, seed=11)
    check("shape", x, template, [torch.tensor([pval])], lpl.to(DEV))
    check("camera", x, template, [torch.tensor([pval]), torch.tensor([-pval / 2])])


def _edge_template(H, W, align, seed=0):
    """points outside [-1,1] (zero padding, partly and wholly outside) and points exactly on pixel centres"""
    g = torch.Generator().manual_seed(seed)
    out = torch.rand(200, 2, generator=g) * 3.2 - 1.6
    if align:
        cx, cy = -1 + 2 * torch.arange(W) / max(W - 1, 1), -1 + 2 * torch.arange(H) / max(H - 1, 1)
    else:
        cx, cy = -1 + (2 * torch.arange(W) + 1) / W, -1 + (2 * torch.arange(H) + 1) / H
    centres = torch.stack(torch.meshgrid(cx, cy, indexing="xy"), -1).reshape(-1, 2)
    xy = torch.cat((out, centres, torch.tensor([[5.0, 0.0], [0.0, -9.0], [1.0, 1.0], [-1.0, -1.0]])))
    return torch.cat((xy, torch.rand(xy.shape[0], 1, generator=g)), 1)[None].float()


def test_points_outside_and_on_pixel_centres():
    x = rand_x(2, 5, 6, 5, seed=2)
    t = _edge_template(6, 5, True)
    V = t.shape[1]
    lpl = torch.randn(V, V) * (torch.rand(V, V) < 0.03)
    check("shape", x, t, [torch.tensor([0.4])], lpl.to(DEV))
    check("camera", x, _edge_template(6, 5, False), [torch.tensor([0.4]), torch.tensor([-1.2])])


def test_fully_dense_lpl():
    template, _ = template_lpl("sphere")
    lpl = torch.randn(642, 642, generator=torch.Generator().manual_seed(4)) / 25
    check("shape", rand_x(2, 6, 4, 4, seed=3), template, [torch.tensor([0.1])], lpl)          # a host lpl, too


@pytest.mark.parametrize("H,W", [(1, 1), (1, 3), (3, 1), (3, 5), (33, 40)])
def test_small_odd_and_large_maps(H, W):
    template, lpl = template_lpl("sphere")
    x = rand_x(2, 4, H, W, seed=H * 7 + W)
    check("shape", x, template, [torch.tensor([-0.5])], lpl.to(DEV))
    check("camera", x, template, [torch.tensor([0.9]), torch.tensor([-0.2])])


def test_odd_vertex_count_bins():
    template, _ = template_lpl("sphere")
    t = template[:, :641]
    check("camera", rand_x(2, 3, 5, 3, seed=9), t, [torch.tensor([0.2]), torch.tensor([0.6])])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_inputs(dtype):
    """fp32 out and a gradient in x's dtype: the same kernels on the same values, so the fp32 path's results bit for bit (its
    gradient rounded once to dtype), which the float64 reference then holds to the fp32 bar"""
    template, lpl = template_lpl("sphere")
    x = rand_x(3, 8, 4, 4, seed=21).to(dtype)
    gen = torch.Generator().manual_seed(1)
    for op, params, shape in (("shape", [torch.tensor([0.3])], (3, 27, 642)), ("camera", [torch.tensor([0.3]), torch.tensor([-1.0])], (3, 16, 2, 2))):
        extra = (lpl.to(DEV),) if op == "shape" else ()
        g = torch.randn(shape, generator=gen)
        out_h, gx_h, gp_h = _run(op, x, template, params, g, extra)
        out_f, gx_f, gp_f = _run(op, x.float(), template, params, g, extra)
        assert out_h.dtype == torch.float32 and gx_h.dtype == dtype
        assert torch.equal(out_h, out_f) and torch.equal(gx_h, gx_f.to(dtype))
        for a, b in zip(gp_h, gp_f):
            assert torch.equal(a, b)
        # against the float64 reference on x's values: the bar, widened for x's gradient by its one rounding to dtype
        check(op, x, template, params, *extra, grad_bar=max(GRAD_BAR, torch.finfo(dtype).eps))


def test_strided_input():
    template, lpl = template_lpl("sphere")
    base = rand_x(3, 10, 6, 9, seed=8)
    x = base[:, ::2, 1:5, ::2]                                         # (3,5,4,5), no unit stride
    xc = base.contiguous(memory_format=torch.channels_last)
    check("shape", x, template, [torch.tensor([0.0])], lpl.to(DEV))
    check("camera", x, template, [torch.tensor([0.0]), torch.tensor([1.0])])
    a = EF.shape_features(xc.to(DEV), template.to(DEV), lpl.to(DEV), torch.tensor([0.2], device=DEV))
    b = EF.shape_features(base.to(DEV), template.to(DEV), lpl.to(DEV), torch.tensor([0.2], device=DEV))
    assert torch.equal(a, b)


def test_max_ties_go_where_torch_sends_them():
    """equal maxima in a bin: the gradient lands on the first in row-major order, as ATen's adaptive_max_pool2d"""
    template, lpl = template_lpl("sphere")
    x = rand_x(2, 3, 5, 6, seed=1) * 0.1
    x[0, 0, 1, 2] = x[0, 0, 3, 1] = x[0, 0, 4, 5] = 2.0              # one global maximum three times
    x[1, 2, 0, 1] = x[1, 2, 0, 2] = x[1, 2, 2, 1] = 3.0              # ties inside the 2x2 bins too (bins of a 5x6 map overlap)
    x[1, 1] = 0.5                                                     # a constant plane
    for op, params, extra in (("shape", [torch.tensor([3.0])], (lpl.to(DEV),)), ("camera", [torch.tensor([3.0]), torch.tensor([2.0])], ())):
        check(op, x, template, params, *extra)                        # the float64 reference pools with ATen: first maximum wins
        xt = x.double().requires_grad_()                                 # where the reference's pool sends a tie
        torch.nn.functional.adaptive_max_pool2d(xt, (1, 1) if op == "shape" else (2, 2)).sum().backward()
        if op == "shape":                                              # one bin: the first of the three, and (0, 0) of the constant plane
            assert xt.grad[0, 0, 1, 2] != 0 and xt.grad[0, 0, 3, 1] == 0 and xt.grad[0, 0, 4, 5] == 0 and xt.grad[1, 1, 0, 0] != 0
        else:                                                          # bin (0, 0) = rows 0-2 x cols 0-2 holds (0,1), (0,2), (2,1)
            assert xt.grad[1, 2, 0, 1] != 0 and xt.grad[1, 2, 0, 2] == 0


def test_bitwise_reproducible():
    template, lpl = template_lpl("smpl_uv_642")
    x = rand_x(8, 64, 4, 4, seed=17)
    runs = []
    for _ in range(2):
        rs = []
        for op, params, extra in (("shape", [torch.tensor([0.3])], (lpl.to(DEV),)), ("camera", [torch.tensor([0.3]), torch.tensor([-1.0])], ())):
            shape = (8, 195, 642) if op == "shape" else (8, 128, 2, 2)
            g = torch.randn(shape, generator=torch.Generator().manual_seed(2))
            out, gx, gp = _run(op, x, template, params, g, extra)
            rs += [out, gx] + gp
        runs.append(rs)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_template_and_lpl_edits_are_picked_up():
    template, lpl = template_lpl("sphere")
    t, L = template.to(DEV), lpl.to(DEV)
    x, p = rand_x(2, 3, 4, 4).to(DEV), torch.tensor([0.1], device=DEV)

    def both():
        return EF.shape_features(x, t, L, p), EF.camera_features(x, t, p, p)

    def ref():
        return (shape_ref(x.cpu().double(), t.cpu(), L.cpu(), p.cpu().double()), camera_ref(x.cpu().double(), t.cpu(), p.cpu().double(), p.cpu().double()))

    def agree():
        for a, b in zip(both(), ref()):
            _close(a, b, FWD_BAR, "forward")

    agree()
    t[0, :100, 0] += 0.3                                              # in-place template edit
    agree()
    t.data = torch.flip(t.data, [1]).contiguous()                     # .data reassignment
    agree()
    L[:, 5] = 0
    L[17, 5] = 2.5                                                    # in-place lpl edit
    agree()
    L.data = L.data * -1.5
    agree()


def test_lpl_requiring_grad_raises():
    template, lpl = template_lpl("sphere")
    with pytest.raises(RuntimeError, match="requires grad"):
        EF.shape_features(rand_x(1, 2, 4, 4).to(DEV), template.to(DEV), lpl.to(DEV).requires_grad_(), torch.zeros(1, device=DEV))


def test_no_grad_and_autocast():
    template, lpl = template_lpl("sphere")
    x = rand_x(2, 4, 4, 4).to(DEV).requires_grad_()
    p = torch.tensor([0.5], device=DEV, requires_grad=True)
    with torch.no_grad():
        a = EF.shape_features(x, template.to(DEV), lpl.to(DEV), p)
        c = EF.camera_features(x, template.to(DEV), p, p)
    assert a.grad_fn is None and c.grad_fn is None and not a.requires_grad
    ref = shape_ref(x.detach().cpu().double(), template, lpl, p.detach().cpu().double())
    _close(a, ref, FWD_BAR, "no_grad forward")
    with torch.autocast("cuda", dtype=torch.float16):
        xh = torch.nn.functional.conv2d(x, torch.eye(4, device=DEV).reshape(4, 4, 1, 1))     # an fp16 backbone output
        s = EF.shape_features(xh, template.to(DEV), lpl.to(DEV), p)
        cc = EF.camera_features(xh, template.to(DEV), p, p)
    assert xh.dtype == torch.float16 and s.dtype == cc.dtype == torch.float32
    (s.sum() + cc.sum()).backward()
    assert x.grad is not None and x.grad.dtype == torch.float32 and p.grad is not None and torch.isfinite(x.grad).all()
