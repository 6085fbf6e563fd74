"""SSIM / MS-SSIM on the MI355X (csrc/mm_ssim.hip through ssim.py) at the edges of its tiles and in the regime the evaluation runs in:
objects on a flat background, 8-bit-valued, where sigma^2 = E[x^2] - mu^2 cancels against C2 and fp32 is 1e-4 from float64 by
upstream's own arithmetic.  tests/test_gpu_ssim.py holds the kernels to float64 on noise; no float64 bar can be applied on renders, so
here the kernels are held to the fp32 RESTATEMENT of their documented order (tests/test_ssim_host.py: ssim32_maps), which is expected
to give the kernels' per-pixel maps bit for bit.  Only the order of the plane sum differs, and that is bounded, not fitted.

The bound of the plane sum.  u = 2^-24.  A sum of the values x_i along a tree whose longest path has d rounded additions is within
d u sum|x_i| of the exact sum (first order in u; every term carries at most d factors (1 + delta)); the division by P adds one more
rounding.  So a per-channel value is within (d + 1) u mean|map| of the float64 mean of the same fp32 map.  d, read from the code, from a
pixel to the division (an addition to a literal 0 is exact and is not counted; adding the 0 of a masked pixel, lane or wave is exact
too, but the fixed-shape stages are counted whole):

    the thread's values     a thread owns column tid & 63 and rows (tid >> 6) + 4 j, j = 0..3, of a 64x16 tile: with r = min(Ho, 16) live
                            rows the first wave has ceil(r / 4) values, summed into a 0:                    ceil(r / 4) - 1 additions
    the wave butterfly      wave_sum: four DPP steps, then (l0 + l16) + (l32 + l48):                        6
    the four waves          (red[0] + red[1]) + (red[2] + red[3]):                                          2
    the fold's lane run     lane l adds the partials of tiles l, l + 64, ... into a 0: with T = ntx nty tiles ceil(T / 64) - 1
    the second butterfly    wave_sum again:                                                                 6

    d = ceil(min(Ho, 16) / 4) + 12 + ceil(T / 64)        (17 for one full tile row and up to 64 tiles, 18 for the 70 tiles of 220x330)

``ssim(size_average=False)`` then sums the C channel values of an image into a 0 (C - 1 additions) and divides by C: within
(d + 1 + C) u M of the mean of the restated channel values, M the mean over the channels of mean|ssim_map| (which bounds every channel
value).  None of this was tuned on a GPU result: if a case misses, the restatement's order or the kernel is wrong.

Against float64 the suite's <= 1e-5 bar applies wherever the restatement is itself within 5e-6 of float64; elsewhere the case is a
conditioning case, judged by the bound alone, and its distance to float64 is printed (profiles/ssim_conditioning.md keeps the table).

Gradients go through parity_bar.grad_close with the torch-fp32 host autograd as the reference and ssim64's as ref64 (the COND rule,
unchanged).  "cond" is admissible only for render-like inputs whose two backgrounds differ or that are 8-bit at data_range=255; every
noise case and every render-like case on identical backgrounds must be "ok"."""
import functools
import importlib
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import TEMPLATES
from parity_bar import grad_close, rel_errors
from test_export_host import export_images_restated
from test_ssim_host import gauss_taps, ms_ssim_ref, noise_pair, render_like, ssim32_maps, ssim64, ssim_ref, ssim_ref_dtype

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24

# name: (shape, window arguments) -- each the smallest shape that reaches its branch (win_size 11 unless named)
CASES = {
    "anchor": ((2, 3, 64, 80), {}),                                        # the existing regime, for the render-like inputs
    "gather_2x2": ((1, 2, 20, 70), {}),                                    # 1 output tile, 2 x 2 gather tiles
    "one_live_column": ((1, 1, 26, 75), {}),                               # Ho = 16: exactly one tile row; Wo = 65: a second tile with one live column
    "fold_second_trip": ((1, 1, 220, 330), {}),                            # 14 x 5 = 70 tiles
    "w_below_win": ((2, 1, 90, 7), {}),                                    # W < win <= H
    "unfiltered": ((1, 2, 5, 9), {}),                                      # neither dimension filtered
    "win1": ((1, 2, 17, 65), dict(win_size=1)),
    "win3": ((1, 2, 17, 65), dict(win_size=3, win_sigma=0.5)),
    "win31": ((1, 2, 40, 100), dict(win_size=31, win_sigma=4.0)),          # the 39.7 KiB LDS request
    "planes35": ((7, 5, 12, 12), {}),                                      # 35 planes: not a multiple of the fold's 16 waves
}
# kind: (background of X, of Y, levels, data_range); None backgrounds: the noise pair
KINDS = {
    "noise": (None, None, None, 1.0),
    "render": (1.0, 1.0, 255, 1.0),                                        # what export_images(as_float=True) hands the evaluation
    "render_bg": (1.0, 0.98, None, 1.0),                                   # two backgrounds: sigma^2 cancels in both images, apart
    "render_255": (1.0, 0.98, 255, 255.0),                                 # 8-bit values at data_range=255
}
COND_ADMISSIBLE = ("render_bg", "render_255")
GRID = [(c, k) for c in CASES for k in ("noise", "render")] + [("anchor", "render_bg"), ("anchor", "render_255")]
IDS = ["%s-%s" % ck for ck in GRID]


@pytest.fixture(scope="module")
def S():
    return importlib.import_module("3d-magic-mirror_amd.ssim")


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def sum_depth(Ho, Wo):
    """d of the module docstring"""
    tiles = -(-Wo // 64) * -(-Ho // 16)
    return -(-min(Ho, 16) // 4) + 12 + -(-tiles // 64)


@functools.lru_cache(maxsize=None)
def case(name, kind, K=(0.01, 0.03)):
    """inputs and host references of one case, computed once and shared (nothing below writes into them)"""
    shape, win = CASES[name]
    bg_x, bg_y, levels, data_range = KINDS[kind]
    seed = sum(shape) + len(name)
    if bg_x is None:
        X, Y = noise_pair(shape, seed=seed)
    else:
        X, Y = render_like(*shape, seed=seed, bg_x=bg_x, bg_y=bg_y, levels=levels)
    if data_range != 1.0:
        X, Y = X * data_range, Y * data_range                              # exact k for 8-bit values: fl(fl(k / 255) 255) = k
        assert torch.equal(X, torch.round(X)) and torch.equal(Y, torch.round(Y))
    k, sigma = win.get("win_size", 11), win.get("win_sigma", 1.5)
    taps = gauss_taps(k, sigma)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    s_map, c_map = ssim32_maps(X, Y, taps, C1, C2)
    s64, c64 = ssim64(X, Y, taps, C1, C2)
    Ho, Wo = s_map.shape[2:]
    return dict(X=X, Y=Y, kw=dict(data_range=data_range, K=K, **win), taps=taps, C1=C1, C2=C2, d=sum_depth(Ho, Wo),
                s32=s_map.astype(np.float64).mean(axis=(2, 3)), c32=c_map.astype(np.float64).mean(axis=(2, 3)),
                s_abs=np.abs(s_map).astype(np.float64).mean(axis=(2, 3)), c_abs=np.abs(c_map).astype(np.float64).mean(axis=(2, 3)),
                s64=s64.numpy(), c64=c64.numpy())


def test_sum_depth_of_the_cases():
    """the d of every case, by hand from the module docstring's table"""
    want = {"anchor": 17, "gather_2x2": 16, "one_live_column": 17, "fold_second_trip": 18, "w_below_win": 17, "unfiltered": 15,
            "win1": 17, "win3": 17, "win31": 16, "planes35": 14}
    for name, (shape, win) in CASES.items():
        k = win.get("win_size", 11)
        Ho, Wo = (shape[2] - k + 1 if shape[2] >= k else shape[2]), (shape[3] - k + 1 if shape[3] >= k else shape[3])
        assert sum_depth(Ho, Wo) == want[name], name
    assert sum_depth(210, 320) == 18 and -(-320 // 64) * -(-210 // 16) == 70


# ---- values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", GRID, ids=IDS)
def test_values_against_the_restatement_and_float64(S, name, kind):
    c = case(name, kind)
    Xd, Yd = c["X"].to(DEV), c["Y"].to(DEV)
    C = Xd.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                    # the skip rule's warning
        per_image, s_pc, cs_pc = S._SsimFn.apply(Xd, Yd, c["taps"].tolist(), c["C1"], c["C2"], False, True)
        api = S.ssim(Xd, Yd, size_average=False, **c["kw"])
    assert (bits(api) == bits(per_image)).all()                            # the public call is this op
    s_pc, cs_pc, per_image = s_pc.cpu().double().numpy(), cs_pc.cpu().double().numpy(), per_image.cpu().double().numpy()
    d = c["d"]
    # (1) against the restatement, under the bound of the kernel's own summation tree
    e_s, b_s = np.abs(s_pc - c["s32"]), (d + 1) * U * c["s_abs"]
    e_c, b_c = np.abs(cs_pc - c["c32"]), (d + 1) * U * c["c_abs"]
    e_n, b_n = np.abs(per_image - c["s32"].mean(axis=1)), (d + 1 + C) * U * c["s_abs"].mean(axis=1)
    # (2) against float64, where the restatement is itself close to it
    r_s, r_c = float(np.abs(c["s32"] - c["s64"]).max()), float(np.abs(c["c32"] - c["c64"]).max())
    g_s, g_c = float(np.abs(s_pc - c["s64"]).max()), float(np.abs(cs_pc - c["c64"]).max())
    g_n = float(np.abs(per_image - c["s64"].mean(axis=1)).max())
    print("\nSSIM-VALUES | %s | %s | d=%d | restated-f64 ssim %.2e cs %.2e | gpu-restated ssim %.2e (bound %.2e) cs %.2e (bound %.2e) "
          "image %.2e (bound %.2e) | gpu-f64 ssim %.2e cs %.2e image %.2e" % (
              name, kind, d, r_s, r_c, e_s.max(), b_s[np.unravel_index(e_s.argmax(), e_s.shape)], e_c.max(),
              b_c[np.unravel_index(e_c.argmax(), e_c.shape)], e_n.max(), b_n[e_n.argmax()], g_s, g_c, g_n))
    assert (e_s <= b_s).all(), ("ssim per channel", e_s.max(), b_s.min())
    assert (e_c <= b_c).all(), ("cs per channel", e_c.max(), b_c.min())
    assert (e_n <= b_n).all(), ("ssim per image", e_n.max(), b_n.min())
    if r_s <= 5e-6:
        assert g_s <= 1e-5 and g_n <= 1e-5, (g_s, g_n)
    if r_c <= 5e-6:
        assert g_c <= 1e-5, g_c
    if kind == "noise":
        assert r_s <= 5e-6 and r_c <= 5e-6                                 # noise is never a conditioning case


# ---- gradients ------------------------------------------------------------------------------------------------------------------------
def weighted(v):
    """distinct weights per image: no two images' errors can cancel"""
    return (v * torch.arange(1, v.numel() + 1, dtype=v.dtype, device=v.device)).sum()


def gpu_grads(S, X, Y, need=(True, True), **kw):
    Xd, Yd = X.to(DEV).detach().requires_grad_(need[0]), Y.to(DEV).detach().requires_grad_(need[1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        v = S.ssim(Xd, Yd, size_average=False, **kw)
    weighted(v).backward()
    return v.detach(), (None if Xd.grad is None else Xd.grad.cpu()), (None if Yd.grad is None else Yd.grad.cpu())


def host_grads(X, Y, dtype, **kw):
    Xh, Yh = X.detach().to(dtype, copy=True).requires_grad_(True), Y.detach().to(dtype, copy=True).requires_grad_(True)   # the cached case stays as it is
    weighted(ssim_ref_dtype(Xh, Yh, dtype, size_average=False, **kw)).backward()
    return Xh.grad, Yh.grad


def check_gradients(S, name, kind, K=(0.01, 0.03)):
    c = case(name, kind, K)
    _, gx, gy = gpu_grads(S, c["X"], c["Y"], **c["kw"])
    rx, ry = host_grads(c["X"], c["Y"], torch.float32, **c["kw"])
    r64 = functools.lru_cache(maxsize=None)(lambda: host_grads(c["X"], c["Y"], torch.float64, **c["kw"]))
    verdicts = (grad_close(gx, rx, rtol=1e-4, what="%s/%s dX" % (name, kind), ref64=lambda: r64()[0]),
                grad_close(gy, ry, rtol=1e-4, what="%s/%s dY" % (name, kind), ref64=lambda: r64()[1]))
    print("\nSSIM-GRADS | %s | %s | K=%s | dX %s (%.2e of max|ref32|; ref32-f64 %.2e, gpu-f64 %.2e) | dY %s (%.2e; %.2e, %.2e)" % (
        name, kind, K, verdicts[0], rel_errors(gx, rx)[0], rel_errors(rx, r64()[0])[0], rel_errors(gx, r64()[0])[0],
        verdicts[1], rel_errors(gy, ry)[0], rel_errors(ry, r64()[1])[0], rel_errors(gy, r64()[1])[0]))
    if kind not in COND_ADMISSIBLE:
        assert verdicts == ("ok", "ok"), verdicts


@pytest.mark.parametrize("name,kind", GRID, ids=IDS)
def test_gradients(S, name, kind):
    check_gradients(S, name, kind)


def test_gradients_other_constants(S):
    check_gradients(S, "anchor", "noise", K=(0.02, 0.05))


def test_one_sided_gradients_are_the_two_sided_ones(S):
    """only X, then only Y requiring grad (the gather's gy == nullptr / gx == nullptr branches; ssim(pred, gt) is the usual call)"""
    for kind in ("noise", "render"):
        c = case("gather_2x2", kind)
        v, gx, gy = gpu_grads(S, c["X"], c["Y"], **c["kw"])
        vx, gx1, none_y = gpu_grads(S, c["X"], c["Y"], need=(True, False), **c["kw"])
        vy, none_x, gy1 = gpu_grads(S, c["X"], c["Y"], need=(False, True), **c["kw"])
        assert none_y is None and none_x is None
        assert (bits(vx) == bits(v)).all() and (bits(vy) == bits(v)).all()
        assert (bits(gx1) == bits(gx)).all() and (bits(gy1) == bits(gy)).all()
        assert float(gx.abs().max()) > 0 and float(gy.abs().max()) > 0


# ---- exact properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("anchor", "noise"), ("anchor", "render"), ("gather_2x2", "render"), ("one_live_column", "noise"),
                                       ("w_below_win", "noise"), ("win31", "render"), ("anchor", "render_255")])
def test_identical_images_score_exactly_one_with_exactly_zero_gradients(S, name, kind):
    """cs = L = 1 in every pixel (numerator and denominator are the same fp32 number), a plane sum of ones is exact, and the adjoint's
    cancellations are exact: dL/dm = 0, a_xy = -2 a_ee, so 2 x G'a_ee + x G'a_xy = 0"""
    c = case(name, kind)
    v, gx, gy = gpu_grads(S, c["X"], c["X"].clone(), **c["kw"])
    assert (bits(v) == np.float32(1.0).view(np.int32)).all()
    assert ((bits(gx) & 0x7fffffff) == 0).all() and ((bits(gy) & 0x7fffffff) == 0).all()          # a zero, of either sign


@pytest.mark.parametrize("name,kind", [("anchor", "noise"), ("anchor", "render_bg"), ("gather_2x2", "render"), ("w_below_win", "render"),
                                       ("planes35", "noise")])
def test_swapping_the_images_swaps_the_gradients_bit_for_bit(S, name, kind):
    c = case(name, kind)
    v, gx, gy = gpu_grads(S, c["X"], c["Y"], **c["kw"])
    w, hx, hy = gpu_grads(S, c["Y"], c["X"], **c["kw"])
    assert (bits(v) == bits(w)).all()
    assert (bits(gx) == bits(hy)).all() and (bits(gy) == bits(hx)).all()
    assert float(gx.abs().max()) > 0


# ---- non-finite planes ----------------------------------------------------------------------------------------------------------------
def test_a_nan_image_stays_in_its_own_image_and_survives_nonnegative_ssim(S):
    """One NaN pixel (a diverged render) in one channel of image 1 of a batch of 4.  A NaN is plain data here: SSIM derives no address
    from a pixel value."""
    X, Y = noise_pair((4, 3, 40, 52), seed=17)
    Xn = X.clone()
    Xn[1, 2, 20, 30] = float("nan")
    others = [0, 2, 3]
    box = torch.zeros(4, 3, 40, 52, dtype=torch.bool)
    box[1, 2, 10:31, 20:41] = True                                         # every pixel that shares a window with the NaN
    for nonneg in (False, True):
        kw = dict(data_range=1, nonnegative_ssim=nonneg)
        v, gx, gy = gpu_grads(S, X, Y, **kw)
        vn, gxn, gyn = gpu_grads(S, Xn, Y, **kw)
        assert torch.isnan(vn.cpu()).tolist() == [False, True, False, False], (nonneg, vn)      # relu keeps a NaN, as torch.relu does
        assert (bits(vn[others]) == bits(v[others])).all()
        assert (bits(gxn[others]) == bits(gx[others])).all() and (bits(gyn[others]) == bits(gy[others])).all()
        assert bool(torch.isnan(S.ssim(Xn.to(DEV), Y.to(DEV), size_average=True, **kw)))
        # image 1: what torch.relu over the float64 restatement gives -- the gradient is passed through (NaN where a window holds the
        # NaN, the float64 gradient everywhere else, the image's two clean channels included)
        X64, Y64 = Xn.double().requires_grad_(True), Y.double().requires_grad_(True)
        weighted(ssim_ref(X64, Y64, size_average=False, **kw)).backward()
        for got, ref, what in ((gxn, X64.grad, "dX"), (gyn, Y64.grad, "dY")):
            assert torch.equal(torch.isnan(ref), box)
            assert torch.equal(torch.isnan(got), box), (nonneg, what, int(torch.isnan(got).sum()))
            assert float(got[1, :2].abs().max()) > 0
            grad_close(torch.nan_to_num(got[1], nan=0.0), torch.nan_to_num(ref[1], nan=0.0), what="nan image " + what)


# ---- MS-SSIM at odd sizes (avg_pool2d's padding branch) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 161, 175), (1, 1, 163, 162)])
def test_ms_ssim_at_odd_sizes(S, shape):
    X, Y = noise_pair(shape, seed=shape[2])                                # every level's cs is positive: tests/test_ssim_host.py checks it
    Xd, Yd = X.to(DEV).requires_grad_(True), Y.to(DEV).requires_grad_(True)
    got = S.ms_ssim(Xd, Yd, data_range=1, size_average=False)
    ref = ms_ssim_ref(X, Y, data_range=1, size_average=False)
    err = float((got.detach().cpu().double() - ref).abs().max())
    print("\nSSIM-MS | %s | gpu-f64 %.2e" % (shape, err))
    assert err <= 1e-5
    assert abs(float(S.ms_ssim(X.to(DEV), Y.to(DEV), data_range=1)) - float(ms_ssim_ref(X, Y, data_range=1))) <= 1e-5
    weighted(got).backward()
    X64, Y64 = X.double().requires_grad_(True), Y.double().requires_grad_(True)
    weighted(ms_ssim_ref(X64, Y64, data_range=1, size_average=False)).backward()
    print("SSIM-MS-GRADS | %s | dX %.2e dY %.2e of max|f64|" % (shape, rel_errors(Xd.grad, X64.grad)[0], rel_errors(Yd.grad, Y64.grad)[0]))
    assert grad_close(Xd.grad, X64.grad, what="ms_ssim dX") == "ok" and grad_close(Yd.grad, Y64.grad, what="ms_ssim dY") == "ok"


# ---- the evaluation chain: render -> 8-bit export -> recon_scores ------------------------------------------------------------------------
def iou_bound(npix):
    """mask_iou_sums_kernel sums npix terms per image: ceil(npix / 1024) per thread into a 0, wave_sum (6), sixteen wave totals into a 0
    (15); a term of the numerator carries one rounding (l r), of the denominator three; all terms are >= 0, so each sum's relative error
    is at most (additions + roundings of a term) u.  The quotient adds those of the two sums, the rounding of + 1e-10 and its own."""
    adds = -(-npix // 1024) - 1 + 6 + 15
    return ((adds + 1) + (adds + 3) + 2) * U


def test_evaluation_chain_render_export_scores(S, pkg):
    B, side = 3, 64
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), side)
    att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, B, side, side, seed=4)
    datt = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in att.items()}
    with torch.no_grad():
        rgbs, _ = dr.render(no_mask=True, **datt)
    images = []
    for x in (rgbs, gt.to(DEV)):
        rgb, mask = pkg.export_images(x, "rgb+mask", as_float=True)
        r_rgb, r_mask = export_images_restated(x.cpu(), "rgb+mask", float_=True)
        assert torch.equal(rgb.cpu(), r_rgb) and torch.equal(mask.cpu(), r_mask)                   # (tests/test_gpu_export.py's subject)
        images.append((torch.cat((rgb, mask[:, None]), 1), torch.cat((r_rgb, r_mask[:, None]), 1)))
    (pred, r_pred), (gt8, r_gt) = images
    s, iou = S.recon_scores(pred, gt8)
    assert s.shape == (B,) and iou.shape == (B,)
    # ssim: against the restatement of the restated export, under the bound of the module docstring
    taps = gauss_taps(11, 1.5)
    s_map, _ = ssim32_maps(r_pred[:, :3], r_gt[:, :3], taps, 0.01 ** 2, 0.03 ** 2)
    restated = s_map.astype(np.float64).mean(axis=(1, 2, 3))
    d = sum_depth(side - 10, side - 10)
    bound = (d + 1 + 3) * U * np.abs(s_map).astype(np.float64).mean(axis=(1, 2, 3))
    err = np.abs(s.cpu().double().numpy() - restated)
    f64 = ssim_ref(r_pred[:, :3], r_gt[:, :3], data_range=1, size_average=False).numpy()
    # the IoU: against float64
    l, r = r_gt[:, 3].double().flatten(1), r_pred[:, 3].double().flatten(1)
    iou64 = ((l * r).sum(1) / ((l + r - l * r).sum(1) + 1e-10)).numpy()
    iou_err = np.abs(iou.cpu().double().numpy() - iou64)
    print("\nSSIM-CHAIN | d=%d | restated-f64 %.2e | gpu-restated %.2e (bound %.2e) | gpu-f64 %.2e | iou gpu-f64 %.2e (bound %.2e)" % (
        d, np.abs(restated - f64).max(), err.max(), bound[err.argmax()], np.abs(s.cpu().double().numpy() - f64).max(), iou_err.max(),
        iou_bound(side * side) * iou64[iou_err.argmax()]))
    assert (err <= bound).all(), (err, bound)
    assert (iou64 > 0).any() and (iou_err <= iou_bound(side * side) * iou64).all(), (iou_err, iou64)


def test_iou_of_empty_and_full_masks_is_exact(S):
    g = torch.Generator().manual_seed(5)
    pred, gt = torch.rand(2, 4, 12, 12, generator=g), torch.rand(2, 4, 12, 12, generator=g)
    pred[:, 3], gt[:, 3] = 0.0, 0.0
    _, iou = S.recon_scores(pred.to(DEV), gt.to(DEV))
    assert (bits(iou) == 0).all()                                                                 # 0 / (0 + 1e-10)
    pred[:, 3], gt[:, 3] = 1.0, 1.0
    _, iou = S.recon_scores(pred.to(DEV), gt.to(DEV))
    n = np.float32(144.0)
    assert (bits(iou) == (n / (n + np.float32(1e-10))).view(np.int32)).all()
