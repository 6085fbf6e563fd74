"""SSIM (3d-magic-mirror_amd/ssim.py, csrc/mm_ssim.hip) without a GPU: the C ABI's mirror and argument checks, the Python API's checks,
the pytorch_msssim drop-in, and the float64 restatement of pytorch_msssim that tests/test_gpu_ssim.py measures the kernels against."""
import ctypes
import importlib
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

PKG = os.path.join(ROOT, "3d-magic-mirror_amd")


# ---- the float64 restatement (ssim.py's module docstring R1-R9), torch on the host ------------------------------------------------
def gauss_taps(size, sigma):
    """R1 in fp32, as upstream builds it"""
    coords = torch.arange(size, dtype=torch.float32)
    coords -= size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    g /= g.sum()
    return g


def ssim64(X, Y, taps, C1, C2):
    """(ssim per channel, cs per channel) of (N,C,H,W) images in float64 (R2, R4-R6); taps: 1-D"""
    X, Y = X.double(), Y.double()
    C = X.shape[1]
    k = taps.numel()
    w = taps.double().reshape(1, 1, 1, k).repeat(C, 1, 1, 1)

    def filt(t):
        if t.shape[2] >= k:
            t = F.conv2d(t, w.transpose(2, 3), groups=C)
        if t.shape[3] >= k:
            t = F.conv2d(t, w, groups=C)
        return t

    mx, my = filt(X), filt(Y)
    sx2, sy2, sxy = filt(X * X) - mx * mx, filt(Y * Y) - my * my, filt(X * Y) - mx * my
    cs_map = (2 * sxy + C2) / (sx2 + sy2 + C2)
    ssim_map = (2 * mx * my + C1) / (mx * mx + my * my + C1) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def ssim_ref(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False):
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    s, _ = ssim64(X, Y, gauss_taps(win_size, win_sigma), C1, C2)
    if nonnegative_ssim:
        s = torch.relu(s)
    return s.mean() if size_average else s.mean(1)


def ms_ssim_ref(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    """R9 in float64"""
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    taps = gauss_taps(win_size, win_sigma)
    X, Y = X.double(), Y.double()
    w = torch.tensor([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], dtype=torch.float64)
    mcs = []
    for i in range(5):
        s, cs = ssim64(X, Y, taps, C1, C2)
        if i < 4:
            mcs.append(torch.relu(cs))
            pad = [d % 2 for d in X.shape[2:]]
            X = F.avg_pool2d(X, kernel_size=2, padding=pad)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=pad)
    v = torch.prod(torch.stack(mcs + [torch.relu(s)], 0) ** w.view(-1, 1, 1), dim=0)
    return v.mean() if size_average else v.mean(1)


# ---- the fp32 restatement of the forward: the kernels' documented order, stated without their text ---------------------------------
def ssim32_maps(X, Y, taps, C1, C2):
    """(ssim_map, cs_map), float32 (N,C,Ho,Wo), of (N,C,H,W) images with float32 at EVERY step (numpy: one rounding per operation, no
    fused multiply-add), in the order csrc/mm_ssim.hip documents: per moment m in (x, y, x*x, y*y, x*y) the vertical pass
    a = fl(a + fl(vt[t] * m)), t = 0..kh-1, from 0, then the horizontal pass the same way over ht, then R4-R5 in upstream's order.
    A dimension shorter than the window has one tap of 1 (R2's skip rule).  The float64 means of the two maps are "the restated value":
    the kernels are built with -ffp-contract=off and IEEE division, so their maps are expected to BE these maps and only the order of
    the plane sum differs."""
    f32 = np.float32
    X = np.ascontiguousarray(X.detach().cpu().numpy() if torch.is_tensor(X) else X, dtype=f32)
    Y = np.ascontiguousarray(Y.detach().cpu().numpy() if torch.is_tensor(Y) else Y, dtype=f32)
    taps = np.asarray(taps.detach().cpu().numpy() if torch.is_tensor(taps) else taps, dtype=f32)
    assert X.shape == Y.shape and X.ndim == 4 and taps.ndim == 1
    k, (H, W) = taps.shape[0], X.shape[2:]
    one = np.ones(1, f32)
    vt = taps if H >= k else one
    ht = taps if W >= k else one
    C1, C2 = f32(C1), f32(C2)

    def filt(m):
        assert m.dtype == f32
        Ho, Wo = H - len(vt) + 1, W - len(ht) + 1
        a = np.zeros(m.shape[:2] + (Ho, W), f32)
        for t in range(len(vt)):
            a = a + vt[t] * m[:, :, t:t + Ho, :]
        b = np.zeros(m.shape[:2] + (Ho, Wo), f32)
        for t in range(len(ht)):
            b = b + ht[t] * a[:, :, :, t:t + Wo]
        assert b.dtype == f32
        return b

    with np.errstate(all="ignore"):                    # NaN planes are legitimate inputs
        mx, my, exx, eyy, exy = filt(X), filt(Y), filt(X * X), filt(Y * Y), filt(X * Y)
        m1s, m2s, m12 = mx * mx, my * my, mx * my
        s1, s2, s12 = exx - m1s, eyy - m2s, exy - m12
        cs_map = (f32(2) * s12 + C2) / (s1 + s2 + C2)
        ssim_map = ((f32(2) * m12 + C1) / (m1s + m2s + C1)) * cs_map
    assert ssim_map.dtype == f32 and cs_map.dtype == f32
    return ssim_map, cs_map


def ssim32(X, Y, taps, C1, C2):
    """the restated value: (ssim per channel, cs per channel), float64 (N,C) means of ssim32_maps"""
    s, c = ssim32_maps(X, Y, taps, C1, C2)
    return s.astype(np.float64).mean(axis=(2, 3)), c.astype(np.float64).mean(axis=(2, 3))


def ssim_torch(X, Y, taps, C1, C2, dtype):
    """ssim64's formula in ``dtype`` on the host, differentiable: with torch.float32 it is the fp32 reference for GRADIENTS (the ref of
    parity_bar.grad_close, beside ssim64's as ref64)"""
    X, Y = X.to(dtype), Y.to(dtype)
    C = X.shape[1]
    k = taps.numel()
    w = taps.to(dtype).reshape(1, 1, 1, k).repeat(C, 1, 1, 1)

    def filt(t):
        if t.shape[2] >= k:
            t = F.conv2d(t, w.transpose(2, 3), groups=C)
        if t.shape[3] >= k:
            t = F.conv2d(t, w, groups=C)
        return t

    mx, my = filt(X), filt(Y)
    sx2, sy2, sxy = filt(X * X) - mx * mx, filt(Y * Y) - my * my, filt(X * Y) - mx * my
    cs_map = (2 * sxy + C2) / (sx2 + sy2 + C2)
    ssim_map = (2 * mx * my + C1) / (mx * mx + my * my + C1) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def ssim_ref_dtype(X, Y, dtype, data_range=255, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False):
    """ssim_ref evaluated in ``dtype``"""
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    s, _ = ssim_torch(X, Y, gauss_taps(win_size, win_sigma), C1, C2, dtype)
    if nonnegative_ssim:
        s = torch.relu(s)
    return s.mean() if size_average else s.mean(1)


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------
def noise_pair(shape, seed, scale=1.0, noise=0.15):
    """a seeded uniform-noise image and a noisy copy of it, in [0, scale] (the recipe of tests/test_gpu_ssim.py's pair)"""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(shape, generator=g)
    Y = (0.7 * X + 0.3 * torch.rand(shape, generator=g) + noise * torch.randn(shape, generator=g)).clamp(0, 1)
    return (X * scale).float(), (Y * scale).float()


def render_like(N, C, H, W, seed, bg_x, bg_y, levels=None):
    """What the evaluation scores: an object on a flat background.  Every image is an ellipse of uniform-random texture (semi-axes
    0.3 H and 0.3 W, at least 1, about the centre pixel, so that every shape has textured and flat pixels) on the constant bg_x; Y has
    the ellipse one pixel further down, the texture perturbed by N(0, 0.1) noise and clamped to [0, 1], on bg_y.  levels=255 floors both
    to k/255 (an 8-bit image as export_images(as_float=True) returns it): score with data_range=1, or times 255 with data_range=255."""
    g = torch.Generator().manual_seed(seed)
    ys = torch.arange(H, dtype=torch.float64)[:, None] - (H - 1) / 2.0
    xs = torch.arange(W, dtype=torch.float64)[None, :] - (W - 1) / 2.0
    ay, ax = max(1.0, 0.3 * H), max(1.0, 0.3 * W)
    inside_x = (ys / ay) ** 2 + (xs / ax) ** 2 <= 1.0
    inside_y = ((ys - 1.0) / ay) ** 2 + (xs / ax) ** 2 <= 1.0
    tex = torch.rand(N, C, H, W, generator=g)
    tex_y = (tex + 0.1 * torch.randn(N, C, H, W, generator=g)).clamp(0, 1)
    X = torch.where(inside_x, tex, torch.full_like(tex, bg_x)).float()
    Y = torch.where(inside_y, tex_y, torch.full_like(tex, bg_y)).float()
    if levels is not None:
        lv = torch.full((), float(levels), dtype=torch.float32)
        X, Y = torch.floor(X * lv) / lv, torch.floor(Y * lv) / lv
    return X.contiguous(), Y.contiguous()


# ---- the restatement meets its closed forms ------------------------------------------------------------------------------------
def test_restatement_identical_images_give_one():
    g = torch.Generator().manual_seed(0)
    X = torch.rand(2, 3, 40, 33, generator=g)
    s, cs = ssim64(X, X.clone(), gauss_taps(11, 1.5), 1e-4, 9e-4)
    assert torch.allclose(s, torch.ones_like(s), atol=1e-12) and torch.allclose(cs, torch.ones_like(cs), atol=1e-12)


@pytest.mark.parametrize("c1,c2", [(0.2, 0.7), (0.9, 0.1), (0.5, 0.5)])
def test_restatement_constant_images_closed_form(c1, c2):
    C1, C2 = 1e-4, 9e-4
    X, Y = torch.full((1, 2, 20, 24), c1), torch.full((1, 2, 20, 24), c2)
    X, Y = X.float().double(), Y.float().double()
    taps = gauss_taps(11, 1.5).double()
    taps /= taps.sum()                               # the closed form needs a window of sum 1; the fp32 taps' sum is 1 only to an ulp
    s, cs = ssim64(X, Y, taps, C1, C2)
    a, b = float(X[0, 0, 0, 0]), float(Y[0, 0, 0, 0])
    want = (2 * a * b + C1) / (a * a + b * b + C1)
    assert torch.allclose(cs, torch.ones_like(cs), atol=1e-9)
    assert torch.allclose(s, torch.full_like(s, want), atol=1e-9)


def test_taps_are_the_fp32_construction_bit_for_bit():
    S = importlib.import_module("3d-magic-mirror_amd.ssim")
    for size, sigma in ((11, 1.5), (7, 1.0), (1, 1.5), (31, 4.0)):
        ref = gauss_taps(size, sigma).numpy()
        got = S._fspecial_gauss_1d(size, sigma).reshape(-1).numpy()
        assert got.dtype == np.float32 and got.view(np.int32).tolist() == ref.view(np.int32).tolist()
        # and what goes into the descriptor: the same 32-bit patterns
        X = torch.zeros(1, 1, 40, 40)
        _, _, taps, k = S._prepare(X, X, size, sigma, None)
        d = S._make_desc(X, X, taps, 1e-4, 9e-4, False)
        assert k == size and np.array(d.win[:size], dtype=np.float32).view(np.int32).tolist() == ref.view(np.int32).tolist()
        assert all(v == 0.0 for v in d.win[size:])


# ---- ABI mirror and argument checks --------------------------------------------------------------------------------------------
def test_ssim_symbols_and_structs_are_mirrored_at_the_headers_abi():
    """The SSIM symbols and structs (ABI 7) are mirrored, by a binding and a library at exactly the header's MM_ABI_VERSION (not a
    literal: later additions to the ABI bump it)."""
    N = importlib.import_module("3d-magic-mirror_amd._native")
    lib = N.lib()
    for name in ("mm_ssim_query_workspace", "mm_ssim_forward", "mm_ssim_backward"):
        assert name in N.EXPORTS and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "mm_render.h")).read()
    hdr_version = int(re.search(r"#define MM_ABI_VERSION (\d+)", hdr).group(1))
    assert N.ABI_VERSION == lib.mm_abi_version() == hdr_version >= 7
    assert lib.mm_struct_size(18) == ctypes.sizeof(N.MMSsimDesc) > 0
    assert lib.mm_struct_size(19) == ctypes.sizeof(N.MMSsimGrads) > 0
    assert "#define MM_SSIM_MAX_WIN %d" % N.SSIM_MAX_WIN in hdr and "#define MM_SSIM_NONNEG %d" % N.SSIM_NONNEG in hdr


def _desc(N, Nn=2, C=3, H=32, W=40, k=11):
    d = N.MMSsimDesc()
    d.N, d.C, d.H, d.W, d.win_size = Nn, C, H, W, k
    d.x = d.y = d.ssim = 16                          # never dereferenced: every case below fails before a launch
    return d


def test_abi_rejects_bad_arguments_before_any_launch():
    N = importlib.import_module("3d-magic-mirror_amd._native")
    lib = N.lib()
    d = _desc(N)
    ws = lib.mm_ssim_query_workspace(ctypes.byref(d))
    Ho, Wo = 32 - 10, 40 - 10
    assert ws == (2 * 3 * 4 * Ho * Wo * 4 + 255) // 256 * 256                          # the backward's four adjoint maps
    fwd = lambda d: lib.mm_ssim_forward(ctypes.byref(d), None)                          # noqa: E731
    g = N.MMSsimGrads(16, None, 16, None)
    bwd = lambda d, g=g: lib.mm_ssim_backward(ctypes.byref(d), ctypes.byref(g), None)  # noqa: E731
    assert lib.mm_ssim_forward(None, None) == -1 and lib.mm_ssim_backward(None, None, None) == -1
    assert fwd(d) == -3 and bwd(d) == -3                                                # no workspace
    d.workspace, d.workspace_bytes = 256, ws - 1
    assert fwd(d) == -3
    for field, value in (("win_size", 10), ("win_size", 33), ("win_size", 0), ("N", 0), ("H", -1), ("W", 70000)):
        e = _desc(N)
        setattr(e, field, value)
        e.workspace, e.workspace_bytes = 256, 1 << 40
        assert lib.mm_ssim_query_workspace(ctypes.byref(e)) == 0
        assert fwd(e) == -2 and bwd(e) == -2, (field, value)
    e = _desc(N)
    e.workspace, e.workspace_bytes = 256, ws
    e.x = None
    assert fwd(e) == -1
    e.x, e.ssim = 16, None
    assert fwd(e) == -1
    assert bwd(e, N.MMSsimGrads(None, None, 16, 16)) == -1                              # no upstream gradient
    assert bwd(e, N.MMSsimGrads(16, 16, None, None)) == -1                              # nothing to write


def test_python_argument_checks():
    S = importlib.import_module("3d-magic-mirror_amd.ssim")
    X = torch.rand(1, 3, 32, 32)
    with pytest.raises(ValueError, match="same dimensions"):
        S.ssim(X, torch.rand(1, 3, 32, 31))
    with pytest.raises(ValueError, match="odd"):
        S.ssim(X, X, win_size=10)
    with pytest.raises(ValueError, match="odd"):
        S.ms_ssim(X, X, win=torch.ones(1, 1, 4) / 4)
    with pytest.raises(NotImplementedError, match="5-D"):
        S.ssim(torch.rand(1, 3, 8, 32, 32), torch.rand(1, 3, 8, 32, 32))
    with pytest.raises(TypeError, match="fp32"):
        S.ssim(X.double(), X.double())
    with pytest.raises(TypeError, match="fp32"):
        S.ssim(X.half(), X.half())
    with pytest.raises(AssertionError, match="larger than 160"):
        S.ms_ssim(torch.rand(1, 3, 160, 200), torch.rand(1, 3, 160, 200))
    with pytest.raises(NotImplementedError):
        S.SSIM(spatial_dims=3)


# ---- the pytorch_msssim drop-in ------------------------------------------------------------------------------------------------
def test_pytorch_msssim_dropin_names_and_defaults():
    shim_eval = os.path.join(PKG, "shim_eval")
    assert not os.path.exists(os.path.join(PKG, "shim", "pytorch_msssim"))          # shim/ alone never shadows an installed one
    saved = sys.modules.pop("pytorch_msssim", None)
    sys.path.insert(0, shim_eval)
    try:
        pm = importlib.import_module("pytorch_msssim")
        assert os.path.dirname(pm.__file__) == os.path.join(shim_eval, "pytorch_msssim")
        S = importlib.import_module("3d-magic-mirror_amd.ssim")
        assert pm.ssim is S.ssim and pm.ms_ssim is S.ms_ssim and pm.SSIM is S.SSIM and pm.MS_SSIM is S.MS_SSIM

        def sig(f):
            return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

        e = inspect.Parameter.empty
        assert sig(pm.ssim) == [("X", e), ("Y", e), ("data_range", 255), ("size_average", True), ("win_size", 11), ("win_sigma", 1.5),
                                ("win", None), ("K", (0.01, 0.03)), ("nonnegative_ssim", False)]
        assert sig(pm.ms_ssim) == [("X", e), ("Y", e), ("data_range", 255), ("size_average", True), ("win_size", 11), ("win_sigma", 1.5),
                                   ("win", None), ("weights", None), ("K", (0.01, 0.03))]
        assert sig(pm.SSIM.__init__)[1:] == [("data_range", 255), ("size_average", True), ("win_size", 11), ("win_sigma", 1.5),
                                             ("channel", 3), ("spatial_dims", 2), ("K", (0.01, 0.03)), ("nonnegative_ssim", False)]
        assert sig(pm.MS_SSIM.__init__)[1:] == [("data_range", 255), ("size_average", True), ("win_size", 11), ("win_sigma", 1.5),
                                                ("channel", 3), ("spatial_dims", 2), ("weights", None), ("K", (0.01, 0.03))]
        m = pm.SSIM(channel=4, win_size=7)
        assert tuple(m.win.shape) == (4, 1, 1, 7) and m.win.dtype == torch.float32
    finally:
        sys.path.remove(shim_eval)
        sys.modules.pop("pytorch_msssim", None)
        if saved is not None:
            sys.modules["pytorch_msssim"] = saved


def test_package_reexports():
    pkg = importlib.import_module("3d-magic-mirror_amd")
    S = importlib.import_module("3d-magic-mirror_amd.ssim")
    assert pkg.ssim is S.ssim and pkg.ms_ssim is S.ms_ssim and pkg.SSIM is S.SSIM and pkg.MS_SSIM is S.MS_SSIM
    assert pkg.recon_scores is S.recon_scores
    assert S.MS_WEIGHTS == [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]


# ---- the fp32 restatement and the input generators, checked without a GPU ------------------------------------------------------------
C1_1, C2_1 = 0.01 ** 2, 0.03 ** 2                     # data_range = 1


@pytest.mark.parametrize("shape", [(2, 3, 40, 33), (1, 2, 20, 70), (2, 1, 7, 40), (2, 1, 30, 7), (1, 2, 5, 9)])
def test_restatement32_is_within_1e6_of_float64_on_noise(shape):
    X, Y = noise_pair(shape, seed=sum(shape))
    taps = gauss_taps(11, 1.5)
    s32, c32 = ssim32(X, Y, taps, C1_1, C2_1)
    s64, c64 = ssim64(X, Y, taps, C1_1, C2_1)
    assert np.abs(s32 - s64.numpy()).max() <= 1e-6 and np.abs(c32 - c64.numpy()).max() <= 1e-6


def test_restatement32_honours_the_skip_rule():
    taps = gauss_taps(11, 1.5)
    for shape, out in (((2, 1, 7, 40), (7, 30)), ((2, 1, 30, 7), (20, 7)), ((1, 2, 5, 9), (5, 9)), ((1, 1, 11, 11), (1, 1)), ((1, 1, 10, 11), (10, 1))):
        X, Y = noise_pair(shape, seed=3)
        s, c = ssim32_maps(X, Y, taps, C1_1, C2_1)
        assert s.shape == shape[:2] + out and c.shape == s.shape and s.dtype == np.float32, shape
    # neither dimension filtered: the moments are the pixels themselves, so the maps are R4-R5 on single pixels
    X, Y = noise_pair((1, 2, 5, 9), seed=3)
    s, c = ssim32_maps(X, Y, taps, C1_1, C2_1)
    x, y = X.double(), Y.double()
    assert np.abs(c - 1.0).max() <= 1e-6                                              # sigma = 0 to rounding: cs = C2 / C2
    assert np.abs(s - ((2 * x * y + C1_1) / (x * x + y * y + C1_1)).numpy()).max() <= 1e-5
    # a window of one tap (win_size=1) is the same thing at any size
    X, Y = noise_pair((1, 1, 17, 19), seed=4)
    s1, c1 = ssim32_maps(X, Y, gauss_taps(1, 1.5), C1_1, C2_1)
    assert s1.shape == (1, 1, 17, 19) and float(gauss_taps(1, 1.5)[0]) == 1.0


def test_restatement32_gives_exactly_one_on_identical_images():
    for shape, k, sigma in (((2, 3, 40, 33), 11, 1.5), ((1, 1, 7, 40), 11, 1.5), ((1, 2, 40, 50), 31, 4.0), ((1, 1, 9, 9), 3, 0.5)):
        X, _ = noise_pair(shape, seed=k)
        s, c = ssim32_maps(X, X.clone(), gauss_taps(k, sigma), C1_1, C2_1)
        assert (s.view(np.int32) == np.float32(1.0).view(np.int32)).all() and (c.view(np.int32) == np.float32(1.0).view(np.int32)).all()
    Xr, _ = render_like(1, 2, 40, 33, seed=1, bg_x=1.0, bg_y=1.0, levels=255)
    s, c = ssim32_maps(Xr, Xr.clone(), gauss_taps(11, 1.5), C1_1, C2_1)
    assert (s == 1.0).all() and (c == 1.0).all()


def test_torch_fp32_reference_is_ssim64s_formula():
    X, Y = noise_pair((2, 3, 40, 33), seed=6)
    taps = gauss_taps(11, 1.5)
    s64, c64 = ssim64(X, Y, taps, C1_1, C2_1)
    sd, cd = ssim_torch(X, Y, taps, C1_1, C2_1, torch.float64)
    assert torch.equal(sd, s64) and torch.equal(cd, c64)
    sf, cf = ssim_torch(X, Y, taps, C1_1, C2_1, torch.float32)
    assert sf.dtype == torch.float32 and (sf.double() - s64).abs().max() <= 1e-6 and (cf.double() - c64).abs().max() <= 1e-6
    assert float(ssim_ref_dtype(X, Y, torch.float64, data_range=1)) == float(ssim_ref(X, Y, data_range=1))


@pytest.mark.parametrize("shape", [(2, 3, 64, 80), (1, 2, 20, 70), (1, 1, 26, 75), (2, 1, 90, 7), (1, 2, 5, 9), (1, 2, 17, 65), (7, 5, 12, 12)])
def test_render_like_has_texture_and_flat_background_at_every_shape(shape):
    X, Y = render_like(*shape, seed=2, bg_x=1.0, bg_y=0.98)
    X2, Y2 = render_like(*shape, seed=2, bg_x=1.0, bg_y=0.98)
    assert torch.equal(X, X2) and torch.equal(Y, Y2) and X.dtype == torch.float32 and tuple(X.shape) == shape
    H, W = shape[2:]
    for img, bg in ((X, 1.0), (Y, 0.98)):
        flat = img == np.float32(bg)
        assert bool(flat[:, :, 0, 0].all()) and bool(flat[:, :, -1, -1].all())                    # the corners are background
        assert 0.05 * H * W <= float((~flat[0, 0]).sum()) <= 0.5 * H * W
    assert not bool((X[:, :, H // 2, W // 2] == 1.0).all())                                       # the centre is textured
    assert float(Y.min()) >= 0.0 and float(Y.max()) <= 1.0
    Xq, Yq = render_like(*shape, seed=2, bg_x=1.0, bg_y=0.98, levels=255)
    for q in (Xq, Yq):
        k = torch.round(q * 255)
        assert torch.equal(q, k / torch.full((), 255.0)) and float(k.min()) >= 0 and float(k.max()) <= 255
    assert bool((Xq[:, :, 0, 0] == 1.0).all()) and bool((Yq[:, :, 0, 0] == np.float32(249.0) / np.float32(255.0)).all())


@pytest.mark.parametrize("shape", [(2, 3, 161, 175), (1, 1, 163, 162)])
def test_ms_ssim_reference_cs_is_positive_on_the_odd_noise_pairs(shape):
    """tests/test_gpu_ssim_edges.py differentiates ms_ssim on these pairs: no level may hand ``0 ** w`` to autograd"""
    X, Y = noise_pair(shape, seed=shape[2])
    X, Y = X.double(), Y.double()
    taps = gauss_taps(11, 1.5)
    sizes = []
    for i in range(5):
        s, cs = ssim64(X, Y, taps, C1_1, C2_1)
        assert float(cs.min()) > 0.0 and float(s.min()) > 0.0, i
        sizes.append(tuple(X.shape[2:]))
        pad = [d % 2 for d in X.shape[2:]]
        X, Y = F.avg_pool2d(X, kernel_size=2, padding=pad), F.avg_pool2d(Y, kernel_size=2, padding=pad)
    assert any(h % 2 or w % 2 for h, w in sizes[:4])                                              # the padding branch is taken
    assert min(sizes[4]) >= 11                                                                    # and no level skips a dimension


def test_float64_reference_passes_a_nan_plane_through_relu():
    """what tests/test_gpu_ssim_edges.py holds nonnegative_ssim to: torch.relu keeps a NaN and passes its gradient"""
    X, Y = noise_pair((4, 3, 40, 52), seed=17)
    X[1, 2, 20, 30] = float("nan")
    X64, Y64 = X.double().requires_grad_(True), Y.double().requires_grad_(True)
    v = ssim_ref(X64, Y64, data_range=1, size_average=False, nonnegative_ssim=True)
    assert torch.isnan(v).tolist() == [False, True, False, False]
    (v * torch.arange(1, 5, dtype=v.dtype)).sum().backward()
    box = torch.zeros(4, 3, 40, 52, dtype=torch.bool)
    box[1, 2, 10:31, 20:41] = True                                                                # every pixel that shares a window with the NaN
    assert torch.equal(torch.isnan(X64.grad), box) and torch.equal(torch.isnan(Y64.grad), box)
    assert float(X64.grad[1, :2].abs().max()) > 0.0                                               # the image's other channels keep their gradient
