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
