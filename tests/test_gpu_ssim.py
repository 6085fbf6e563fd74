"""SSIM / MS-SSIM on the MI355X (csrc/mm_ssim.hip through ssim.py) against the float64 restatement of pytorch_msssim kept in
tests/test_ssim_host.py: values within 1e-5, gradients within parity_bar.grad_close, bitwise determinism, batch independence, strided
inputs read in place, host inputs, recon_scores and the pytorch_msssim drop-in."""
import importlib
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, TEMPLATES
from parity_bar import grad_close
from test_ssim_host import ms_ssim_ref, ssim_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def S():
    return importlib.import_module("3d-magic-mirror_amd.ssim")


def pair(shape, seed, scale=1.0, noise=0.15):
    """a seeded image and a noisy, blurred-ish copy of it, in [0, scale]"""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(shape, generator=g)
    Y = (0.7 * X + 0.3 * torch.rand(shape, generator=g) + noise * torch.randn(shape, generator=g)).clamp(0, 1)
    return (X * scale).float(), (Y * scale).float()


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


@pytest.mark.parametrize("shape", [(1, 3, 128, 128), (48, 3, 128, 128), (8, 3, 256, 128), (4, 3, 256, 256), (3, 4, 11, 11), (2, 1, 7, 300)])
def test_forward_matches_float64(S, shape):
    X, Y = pair(shape, seed=sum(shape))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # (2,1,7,300): the skip rule's warning
        got_all = S.ssim(X.to(DEV), Y.to(DEV), data_range=1)
        got_n = S.ssim(X.to(DEV), Y.to(DEV), data_range=1, size_average=False)
    assert got_all.is_cuda and got_all.shape == () and got_n.shape == (shape[0],)
    assert abs(float(got_all) - float(ssim_ref(X, Y, data_range=1))) <= 1e-5
    assert (got_n.cpu().double() - ssim_ref(X, Y, data_range=1, size_average=False)).abs().max() <= 1e-5


def test_forward_window_sigma_constants_and_data_range(S):
    X, Y = pair((4, 3, 96, 80), seed=5, scale=255.0)
    kw = dict(data_range=255, win_size=7, win_sigma=1.0, K=(0.02, 0.05))
    got = S.ssim(X.to(DEV), Y.to(DEV), size_average=False, **kw)
    assert (got.cpu().double() - ssim_ref(X, Y, size_average=False, **kw)).abs().max() <= 1e-5
    # a user-supplied window (pytorch_msssim's (C,1,1,k) layout) is the same window
    w = S._fspecial_gauss_1d(7, 1.0).repeat(3, 1, 1, 1)
    got_w = S.ssim(X.to(DEV), Y.to(DEV), size_average=False, data_range=255, win=w, K=(0.02, 0.05))
    assert (bits(got_w) == bits(got)).all()
    # and the module form
    m = S.SSIM(data_range=255, size_average=False, win_size=7, win_sigma=1.0, channel=3, K=(0.02, 0.05))
    assert (bits(m(X.to(DEV), Y.to(DEV))) == bits(got)).all()


def test_options_size_average_and_nonnegative(S):
    X, _ = pair((3, 3, 64, 64), seed=9)
    Y = 1.0 - X                                           # anti-correlated: negative ssim in every channel
    Y[0] = X[0]                                           # image 0 identical: ssim 1
    ref_n = ssim_ref(X, Y, data_range=1, size_average=False)
    assert float(ref_n[1]) < 0 and float(ref_n[2]) < 0
    got_n = S.ssim(X.to(DEV), Y.to(DEV), data_range=1, size_average=False)
    assert (got_n.cpu().double() - ref_n).abs().max() <= 1e-5
    got = S.ssim(X.to(DEV), Y.to(DEV), data_range=1)
    assert abs(float(got) - float(ref_n.mean())) <= 1e-5
    for sa in (True, False):
        got = S.ssim(X.to(DEV), Y.to(DEV), data_range=1, size_average=sa, nonnegative_ssim=True)
        ref = ssim_ref(X, Y, data_range=1, size_average=sa, nonnegative_ssim=True)
        assert (got.cpu().double() - ref).abs().max() <= 1e-5
    assert abs(float(S.ssim(X.to(DEV), Y.to(DEV), data_range=1, size_average=False, nonnegative_ssim=True)[0]) - 1.0) <= 1e-6


def _grads(fn, X, Y, **kw):
    Xd, Yd = X.to(DEV).detach().requires_grad_(True), Y.to(DEV).detach().requires_grad_(True)
    fn(Xd, Yd, **kw).backward()
    return Xd.grad.cpu(), Yd.grad.cpu()


def _grads64(fn, X, Y, **kw):
    X64, Y64 = X.double().requires_grad_(True), Y.double().requires_grad_(True)
    fn(X64, Y64, **kw).backward()
    return X64.grad, Y64.grad


@pytest.mark.parametrize("shape,kw", [((2, 3, 64, 80), {}), ((3, 2, 40, 52), dict(size_average=False)),
                                      ((2, 3, 48, 48), dict(win_size=7, win_sigma=1.0, K=(0.02, 0.05))),
                                      ((2, 1, 7, 90), {})])
def test_ssim_gradients_match_float64_autograd(S, shape, kw):
    X, Y = pair(shape, seed=3 + shape[2])
    red = (lambda v: (v * torch.arange(1, v.numel() + 1, dtype=v.dtype, device=v.device)).sum()) if kw.get("size_average") is False else (lambda v: v)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gx, gy = _grads(lambda a, b, **k: red(S.ssim(a, b, **k)), X, Y, data_range=1, **kw)
        rx, ry = _grads64(lambda a, b, **k: red(ssim_ref(a, b, **k)), X, Y, data_range=1, **kw)
    grad_close(gx, rx, what="ssim dX"), grad_close(gy, ry, what="ssim dY")


def test_ssim_gradients_nonnegative(S):
    X, Y = pair((2, 3, 48, 48), seed=21)
    Y[1] = 1.0 - X[1]                                     # image 1 below zero: relu cuts its gradient
    gx, gy = _grads(S.ssim, X, Y, data_range=1, nonnegative_ssim=True)
    rx, ry = _grads64(ssim_ref, X, Y, data_range=1, nonnegative_ssim=True)
    assert float(gx[1].abs().max()) == 0.0 and float(gy[1].abs().max()) == 0.0
    grad_close(gx, rx, what="dX"), grad_close(gy, ry, what="dY")


@pytest.mark.parametrize("side", [176, 256])
def test_ms_ssim_forward_and_gradients(S, side):
    X, Y = pair((2, 3, side, side), seed=side)
    got = S.ms_ssim(X.to(DEV), Y.to(DEV), data_range=1)
    assert abs(float(got) - float(ms_ssim_ref(X, Y, data_range=1))) <= 1e-5
    got_n = S.ms_ssim(X.to(DEV), Y.to(DEV), data_range=1, size_average=False)
    assert (got_n.cpu().double() - ms_ssim_ref(X, Y, data_range=1, size_average=False)).abs().max() <= 1e-5
    gx, gy = _grads(S.ms_ssim, X, Y, data_range=1)
    rx, ry = _grads64(ms_ssim_ref, X, Y, data_range=1)
    grad_close(gx, rx, what="ms_ssim dX"), grad_close(gy, ry, what="ms_ssim dY")
    m = S.MS_SSIM(data_range=1, channel=3)
    assert (bits(m(X.to(DEV), Y.to(DEV))) == bits(got)).all()


def test_deterministic_forward_and_backward(S):
    X, Y = pair((48, 3, 128, 128), seed=77)
    outs = []
    for _ in range(2):
        Xd, Yd = X.to(DEV).requires_grad_(True), Y.to(DEV).requires_grad_(True)
        v = S.ssim(Xd, Yd, data_range=1, size_average=False)
        v.sum().backward()
        outs.append((bits(v), bits(Xd.grad), bits(Yd.grad)))
    for a, b in zip(*outs):
        assert (a == b).all()


def test_batch_independence(S):
    X, Y = pair((6, 3, 96, 112), seed=13)
    Xd, Yd = X.to(DEV).requires_grad_(True), Y.to(DEV).requires_grad_(True)
    v = S.ssim(Xd, Yd, data_range=1, size_average=False)
    v.sum().backward()
    for i in range(6):
        xi, yi = X[i:i + 1].to(DEV).requires_grad_(True), Y[i:i + 1].to(DEV).requires_grad_(True)
        vi = S.ssim(xi, yi, data_range=1, size_average=False)
        vi.sum().backward()
        assert (bits(vi) == bits(v[i:i + 1])).all()
        assert (bits(xi.grad) == bits(Xd.grad[i:i + 1])).all() and (bits(yi.grad) == bits(Yd.grad[i:i + 1])).all()


def test_strided_render_output_is_read_in_place(S, pkg):
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), 64)
    att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, 3, 64, 64, seed=4)
    datt = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in att.items()}
    with torch.no_grad():
        rgbs, _ = dr.render(no_mask=True, **datt)
    gt = gt.to(DEV)
    view = rgbs[:, :3]
    assert not view.is_contiguous()
    a = S.ssim(view, gt[:, :3], data_range=1, size_average=False)
    b = S.ssim(view.contiguous(), gt[:, :3].contiguous(), data_range=1, size_average=False)
    assert (bits(a) == bits(b)).all()
    ga = _grads(S.ssim, view, gt[:, :3], data_range=1)
    gb = _grads(S.ssim, view.contiguous(), gt[:, :3].contiguous(), data_range=1)
    assert (bits(ga[0]) == bits(gb[0])).all() and (bits(ga[1]) == bits(gb[1])).all()


def test_host_inputs_give_a_host_result(S):
    X, Y = pair((1, 3, 128, 128), seed=1)
    v = S.ssim(X, Y, data_range=1)
    assert v.device.type == "cpu" and v.shape == ()
    assert (bits(v) == bits(S.ssim(X.to(DEV), Y.to(DEV), data_range=1))).all()
    X, Y = pair((1, 3, 176, 176), seed=1)
    m = S.ms_ssim(X, Y, data_range=1)
    assert m.device.type == "cpu"


def test_recon_scores_equals_the_per_image_loop(S, pkg):
    ops = importlib.import_module("3d-magic-mirror_amd.ops")
    g = torch.Generator().manual_seed(8)
    B, H, W = 5, 80, 96
    pred = torch.rand(B, 4, H, W, generator=g)
    gt = (0.6 * pred + 0.4 * torch.rand(B, 4, H, W, generator=g)).clamp(0, 1)
    pred[:, 3] = (pred[:, 3] > 0.4).float()
    gt[:, 3] = (gt[:, 3] > 0.5).float()
    s, iou = S.recon_scores(pred.to(DEV), gt.to(DEV))
    assert s.shape == (B,) and iou.shape == (B,)
    for i in range(B):
        si = S.ssim(pred[i:i + 1, :3].to(DEV), gt[i:i + 1, :3].to(DEV), data_range=1)
        assert (bits(si) == bits(s[i])).all()
        mi = 1 - ops.mask_iou(gt[i:i + 1, 3].to(DEV), pred[i:i + 1, 3].to(DEV))
        assert abs(float(mi) - float(iou[i])) <= 1e-6
    hs, hi = S.recon_scores(pred, gt)
    assert hs.device.type == "cpu" and (bits(hs) == bits(s)).all() and (bits(hi) == bits(iou)).all()


def test_shim_eval_ssim_is_the_same_function(S):
    shim_eval = os.path.join(ROOT, "3d-magic-mirror_amd", "shim_eval")
    saved = sys.modules.pop("pytorch_msssim", None)
    sys.path.insert(0, shim_eval)
    try:
        pm = importlib.import_module("pytorch_msssim")
        assert pm.ssim is S.ssim
        X, Y = pair((1, 3, 64, 64), seed=2)
        assert (bits(pm.ssim(X, Y, data_range=1)) == bits(S.ssim(X, Y, data_range=1))).all()
    finally:
        sys.path.remove(shim_eval)
        sys.modules.pop("pytorch_msssim", None)
        if saved is not None:
            sys.modules["pytorch_msssim"] = saved


FIXTURE = os.path.join(GOLDEN, "msssim_fixture.npz")


@pytest.mark.skipif(not os.path.exists(FIXTURE), reason="tests/golden/msssim_fixture.npz not minted (tools/mint_msssim_fixture.py)")
def test_matches_real_pytorch_msssim_fixture(S):
    z = np.load(FIXTURE)
    for case in [k[:-2] for k in z.files if k.endswith("_X")]:
        X, Y = torch.from_numpy(z[case + "_X"]), torch.from_numpy(z[case + "_Y"])
        fn = S.ms_ssim if case.startswith("ms") else S.ssim
        Xd, Yd = X.to(DEV).requires_grad_(True), Y.to(DEV).requires_grad_(True)
        v = fn(Xd, Yd, data_range=float(z[case + "_data_range"]), size_average=False)
        assert np.abs(v.detach().cpu().numpy() - z[case + "_val"]).max() <= 1e-5, case
        v.sum().backward()
        grad_close(Xd.grad, z[case + "_gX"], what=case + " dX"), grad_close(Yd.grad, z[case + "_gY"], what=case + " dY")


@pytest.mark.parametrize("rows", (1, 3, 4, 5, 6, 9))
def test_the_written_out_level_product_has_torch_prods_bits(S, rows):
    """ms_ssim multiplies its levels with ssim._prod_rows (torch.prod's backward waits on the host): the forward's bits are torch.prod's,
    on values like the clamped levels raised to their weights, a zero among them; the backward is the product rule, zero factor included"""
    t = torch.rand((rows, 7, 3), generator=torch.Generator().manual_seed(rows)).to(DEV) ** 0.3
    t[rows // 2, 2, 1] = 0.0
    assert (bits(S._prod_rows(t)) == bits(torch.prod(t, dim=0))).all()
    a, b = t.clone().requires_grad_(True), t.double().requires_grad_(True)
    S._prod_rows(a).sum().backward()
    torch.prod(b, dim=0).sum().backward()
    grad_close(a.grad, b.grad, what="product over %d levels" % rows)
