"""Export of renders to 8-bit frames and contact sheets (3d-magic-mirror_amd/export.py, csrc/mm_export.hip) without a GPU: the eager
torch restatement of the quantiser, the composite over white and make_grid that tests/test_gpu_export.py holds the kernels to bit for
bit, with its own self-checks; the C ABI's mirror and argument checks; the Python API's validation and layout choice; and a static
check of the bulk kernels' ISA (16-byte accesses, no scratch, no spills, no LDS).

make_grid is restated from torchvision from memory [recall-risk: torchvision is not installed here, the arithmetic has not been run
against it]."""
import ctypes
import importlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

EX = importlib.import_module("3d-magic-mirror_amd.export")
N = importlib.import_module("3d-magic-mirror_amd._native")


# ---- the restatement (eager torch, CPU, fp32: one rounding per operation) ------------------------------------------------------------
def quantize(x, rounding="trunc"):
    """trunc: fl(x * 255); nearest: fl(fl(x * 255) + 0.5); then NaN -> 0, clamp to [0, 255], toward zero to uint8"""
    q = x.to(torch.float32) * 255.0
    if rounding == "nearest":
        q = q + 0.5
    else:
        assert rounding == "trunc"
    q = torch.where(torch.isnan(q), torch.zeros_like(q), q).clamp(0.0, 255.0)
    return q.to(torch.uint8)


def as_float(q):
    """fl(float(q) / 255): what to_tensor of the saved 8-bit image gives"""
    return q.to(torch.float32) / torch.full((), 255.0, dtype=torch.float32).expand(q.shape)


def white(x):
    """(...,4,H,W): rgb over white with the image's own alpha, fl(fl(rgb * m) + fl(1 - m)); the alpha plane stays"""
    rgb, m = x[..., :3, :, :], x[..., 3:4, :, :]
    return torch.cat((rgb * m + (1 - m), m), -3)


def grid_shape_restated(B, H, W, nrow=8, padding=2):
    if B == 1:
        return H, W
    xmaps = min(nrow, B)
    ymaps = (B + xmaps - 1) // xmaps
    return (H + padding) * ymaps + padding, (W + padding) * xmaps + padding


def make_grid_restated(x, nrow=8, padding=2, pad_value=0.0):
    """torchvision's make_grid for a (B,3,H,W) float tensor -> (3,Hg,Wg)"""
    B, C, H, W = x.shape
    if B == 1:
        return x[0]
    xmaps = min(nrow, B)
    ymaps = (B + xmaps - 1) // xmaps
    grid = x.new_full((C, (H + padding) * ymaps + padding, (W + padding) * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for xx in range(xmaps):
            if k >= B:
                break
            r0, c0 = y * (H + padding) + padding, xx * (W + padding) + padding
            grid[:, r0:r0 + H, c0:c0 + W] = x[k]
            k += 1
    return grid


def export_images_restated(x, channels="rgb", rounding="trunc", white_=False, float_=False):
    """what export.export_images returns, from a CPU (...,C,H,W) tensor"""
    x = x.detach().to(torch.float32)
    if white_:
        x = white(x)
    q = quantize(x, rounding)                                  # (...,C,H,W) uint8
    if float_:
        outs = {"rgb": as_float(q[..., :3, :, :]), "mask": as_float(q[..., 3, :, :]) if q.shape[-3] == 4 else None, "rgba": as_float(q)}
    else:
        hwc = q.movedim(-3, -1)
        outs = {"rgb": hwc[..., :3].contiguous(), "mask": q[..., 3, :, :].contiguous() if q.shape[-3] == 4 else None, "rgba": hwc.contiguous()}
    return (outs["rgb"], outs["mask"]) if channels == "rgb+mask" else outs[channels]


def export_grid_restated(x, nrow=8, padding=2, pad_value=0.0, rounding="trunc", white_=False):
    """what export.export_grid returns, from a CPU (B,C,H,W) or (B,N,C,H,W) tensor"""
    x = x.detach().to(torch.float32)
    if white_:
        x = white(x)
    five = x.dim() == 5
    if not five:
        x = x[:, None]
    frames = [quantize(make_grid_restated(x[:, n, :3], nrow, padding, pad_value).permute(1, 2, 0), rounding).contiguous() for n in range(x.shape[1])]
    return torch.stack(frames) if five else frames[0]


# ---- the restatement's self-checks --------------------------------------------------------------------------------------------------
def test_trunc_is_the_numpy_cast_in_range():
    x = torch.rand(4096, generator=torch.Generator().manual_seed(0))
    x[:3] = torch.tensor([0.0, 1.0, -0.0])
    assert np.array_equal(quantize(x).numpy(), (x * 255).numpy().astype(np.uint8))
    assert np.array_equal(quantize(x).numpy(), (x.numpy() * 255.0).astype(np.uint8))


def test_every_byte_survives_the_round_trip_under_both_roundings():
    k = torch.arange(256, dtype=torch.float32)
    x = as_float(k.to(torch.uint8))
    assert np.array_equal(x.numpy(), (np.arange(256, dtype=np.float32) / np.float32(255.0)))     # bit-exact fp32 division
    for rounding in ("trunc", "nearest"):
        assert int((quantize(x, rounding).to(torch.int64) != torch.arange(256)).sum()) == 0, rounding
        assert torch.equal(as_float(quantize(x, rounding)), x), rounding


def test_quantiser_saturates_and_drops_nan():
    x = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.5, 1.5, -0.0, 1.0, 0.999, 0.5])
    assert quantize(x).tolist() == [0, 255, 0, 0, 255, 0, 255, 254, 127]
    assert quantize(x, "nearest").tolist() == [0, 255, 0, 0, 255, 0, 255, 255, 128]


def test_grid_shapes():
    for (B, kw), want in ((((9), {}), (16, 74)), ((3, {}), (9, 29)), ((1, {}), (5, 7)), ((9, {"padding": 0}), (10, 56))):
        assert grid_shape_restated(B, 5, 7, **kw) == want, (B, kw)
        assert EX.grid_shape(B, 5, 7, **kw) == want, (B, kw)
        assert tuple(export_grid_restated(torch.rand(B, 3, 5, 7), **kw).shape) == want + (3,)
    assert EX.grid_shape(9, 5, 7, nrow=3) == grid_shape_restated(9, 5, 7, nrow=3) == (23, 29)
    for bad in ({"nrow": 0}, {"padding": -1}):
        with pytest.raises(ValueError):
            EX.grid_shape(3, 5, 7, **bad)
    with pytest.raises(ValueError):
        EX.grid_shape(0, 5, 7)


def test_gutters_and_empty_cells_hold_the_quantised_pad_value():
    x = torch.rand(9, 4, 5, 7)
    for pv, rounding, want in ((0.0, "trunc", 0), (1.0, "trunc", 255), (0.5, "trunc", 127), (0.5, "nearest", 128)):
        g = export_grid_restated(x, pad_value=pv, rounding=rounding)
        assert g.shape == (16, 74, 3)
        inside = torch.zeros(16, 74, dtype=torch.bool)
        for k in range(9):
            y, xx = divmod(k, 8)
            r0, c0 = y * 7 + 2, xx * 9 + 2
            inside[r0:r0 + 5, c0:c0 + 7] = True
            assert torch.equal(g[r0:r0 + 5, c0:c0 + 7], quantize(x[k, :3], rounding).permute(1, 2, 0)), k
        assert int(inside.sum()) == 9 * 35 and bool((g[~inside] == want).all()), (pv, rounding)
        assert bool((g[9:14, 11:] == want).all())                                                # the seven empty cells of the second row
    one = export_grid_restated(x[:1], pad_value=1.0)
    assert torch.equal(one, quantize(x[0, :3]).permute(1, 2, 0))                                  # one image: no gutter


def test_white_is_the_composite_of_the_reference():
    x = torch.rand(2, 4, 3, 3)
    w = white(x)
    assert torch.equal(w[:, :3], x[:, :3] * x[:, 3:4] + torch.ones_like(x[:, :3]) * (1 - x[:, 3:4])) and torch.equal(w[:, 3], x[:, 3])
    rgb, mask = export_images_restated(x, "rgb+mask", white_=True)
    assert rgb.shape == (2, 3, 3, 3) and mask.shape == (2, 3, 3) and torch.equal(mask, quantize(x[:, 3]))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_mirrors_the_new_struct_and_symbols(pkg):
    L = N.lib()
    assert N.ABI_VERSION == 9 == L.mm_abi_version()
    assert L.mm_struct_size(29) == ctypes.sizeof(N.MMExportDesc) > 0
    for name in ("mm_export_images", "mm_export_grid"):
        assert name in N.EXPORTS and hasattr(L, name), name


FAKE = ctypes.c_void_p(16)                                # never dereferenced: every call below must fail validation first


def _desc(B=2, Nv=3, C=4, H=8, W=8, **kw):
    d = N.MMExportDesc()
    d.B, d.N, d.C, d.H, d.W = B, Nv, C, H, W
    d.nrow, d.padding = 8, 2
    d.x = d.out_rgb = d.out_grid = FAKE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entry_points_reject_bad_arguments_before_any_launch(pkg):
    L = N.lib()
    img = lambda d: L.mm_export_images(ctypes.byref(d), None)  # noqa: E731
    grid = lambda d: L.mm_export_grid(ctypes.byref(d), None)  # noqa: E731
    assert L.mm_export_images(None, None) == -1 and L.mm_export_grid(None, None) == -1
    assert img(_desc(x=None)) == -1 and grid(_desc(x=None)) == -1 and grid(_desc(out_grid=None)) == -1
    assert img(N.MMExportDesc()) == -2 and grid(N.MMExportDesc()) == -2                           # every size 0
    for call in (img, grid):
        for f in ("B", "N", "H", "W"):
            for v in (0, -3):
                assert call(_desc(**{f: v})) == -2, (f, v)
        for C in (0, 1, 2, 5):
            assert call(_desc(C=C)) == -2, C
        assert call(_desc(C=3, white=1)) == -2
        assert call(_desc(C=3, nhwc=1)) == -2                                                     # NHWC is the 16-byte pixel of a render
        for r in (-1, 2):
            assert call(_desc(rounding=r)) == -2, r
        assert call(_desc(B=1 << 20, H=1 << 12, W=1 << 12)) == -5                                   # the chunk count leaves an int32
    assert img(_desc(out_rgb=None)) == -2                                                         # no output requested
    assert img(_desc(C=3, out_mask=FAKE)) == -2 and img(_desc(C=3, out_rgba=FAKE)) == -2
    assert img(_desc(C=3, out_rgb=None, out_mask=FAKE)) == -2
    for nrow in (0, -1):
        assert grid(_desc(nrow=nrow)) == -2, nrow
    assert grid(_desc(padding=-1)) == -2
    assert grid(_desc(padding=0x7fffffff)) == -5 and grid(_desc(Nv=0x7fffffff, H=64, W=64)) == -5
    assert L.mm_last_error_detail().decode() == ""                                                 # nothing launched, nothing recorded


# ---- the Python API's validation (all of it before any device work) ----------------------------------------------------------------
def test_wrapper_validates_before_anything_reaches_a_kernel(pkg):
    x = torch.rand(2, 4, 4, 4)
    for call in (EX.export_images, EX.export_grid):
        with pytest.raises(RuntimeError, match="device memory"):
            call(x)
        with pytest.raises(RuntimeError, match="device memory"):
            call(torch.rand(2, 3, 4, 4, 4))
        with pytest.raises(ValueError, match="C 3 or 4"):
            call(torch.rand(2, 5, 4, 4))
        with pytest.raises(ValueError, match="C 3 or 4"):
            call(torch.rand(4, 4))
        with pytest.raises(ValueError, match="float tensor"):
            call(x.to(torch.int32))
        with pytest.raises(ValueError, match="float tensor"):
            call(x.numpy())
        with pytest.raises(ValueError, match="rounding"):
            call(x, rounding="floor")
        with pytest.raises(ValueError, match="white"):
            call(x[:, :3], white=True)
    with pytest.raises(ValueError, match=r"\(B,C,H,W\) or \(B,N,C,H,W\)"):
        EX.export_grid(x[0])
    with pytest.raises(ValueError, match=r"\(B,C,H,W\) or \(B,N,C,H,W\)"):
        EX.export_grid(torch.rand(1, 2, 3, 4, 4, 4))
    with pytest.raises(ValueError, match="channels"):
        EX.export_images(x, channels="bgr")
    for ch in ("mask", "rgba", "rgb+mask"):
        with pytest.raises(ValueError, match="4-channel"):
            EX.export_images(x[:, :3], channels=ch)
    with pytest.raises(ValueError, match="nrow"):
        EX.export_grid(x, nrow=0)
    with pytest.raises(ValueError, match="padding"):
        EX.export_grid(x, padding=-1)
    with pytest.raises(RuntimeError, match="device memory"):                                       # a well-formed (C,H,W) image: only the device check is left
        EX.export_images(x[0], channels="rgb+mask", rounding="nearest", white=True, as_float=True)


def test_layout_choice(pkg):
    nchw = torch.rand(2, 4, 4, 4)
    t, f = EX._layout(nchw)
    assert t is nchw and f == 0
    nhwc = torch.rand(2, 4, 4, 4).permute(0, 3, 1, 2)
    t, f = EX._layout(nhwc)
    assert t is nhwc and f == 1 and t.stride() == (64, 1, 16, 4)
    views = torch.rand(2, 3, 5, 7, 4).permute(0, 1, 4, 2, 3)                                       # what render_views returns
    t, f = EX._layout(views)
    assert t is views and f == 1 and t.shape == (2, 3, 4, 5, 7)
    rgb = torch.rand(2, 5, 7, 3).permute(0, 3, 1, 2)                                               # 12-byte pixels: copied
    t, f = EX._layout(rgb)
    assert f == 0 and t.is_contiguous() and torch.equal(t, rgb)
    odd = torch.rand(2, 4, 4, 8)[..., ::2]
    t, f = EX._layout(odd)
    assert f == 0 and t.is_contiguous() and torch.equal(t, odd)
    part = torch.rand(3, 2, 4, 4, 4)[:, 0]                                                         # dense images, strided batch: copied
    t, f = EX._layout(part)
    assert f == 0 and t.is_contiguous() and torch.equal(t, part)


def test_package_exports(pkg):
    assert pkg.export_images is EX.export_images and pkg.export_grid is EX.export_grid and pkg.grid_shape is EX.grid_shape
    import mm_amd
    assert mm_amd.export_grid is EX.export_grid


# ---- the kernels' ISA ---------------------------------------------------------------------------------------------------------------
def _kernels(asm):
    """{mangled name: instructions}, {mangled name: metadata text} of every export kernel in a gfx950 assembly file"""
    lines = asm.splitlines()
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN2mm\w*export_(?:u8|f32|grid)_kernel\w*):", l)
        if not m:
            continue
        end = next(k for k in range(i, len(lines)) if "s_endpgm" in lines[k])
        body = [x.split(";")[0].strip() for x in lines[i + 1:end]]
        out[m.group(1)] = [x for x in body if x and not x.endswith(":") and not x.startswith(".")]
    meta = {}
    for entry in re.split(r"\n  - (?=\.)", asm[asm.index("amdhsa.kernels:"):]):                 # one list item per kernel
        m = re.search(r"^\s+\.name:\s+(\S+)$", entry, flags=re.M)
        if m:
            meta[m.group(1)] = entry
    return out, meta


def test_bulk_instantiations_move_16_bytes_and_use_no_scratch():
    """access width and scratch only.  The byte kernels hold a second path for the bytes around the aligned chunks (the head and tail of a
    sheet, the pixels past the last group of 16): its stores are narrower than a dword, everything else must be a 16-byte access."""
    bn = importlib.import_module("3d-magic-mirror_amd.build_native")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert bn.SOURCES["mm_export.hip"] == bn.EXACT
    src = os.path.join(bn.CSRC, "mm_export.hip")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "export.s")
        subprocess.check_call([hipcc] + bn.FLAGS + bn.SOURCES["mm_export.hip"] + ["-S", "--cuda-device-only", "-o", path, src], stderr=subprocess.DEVNULL)
        asm = open(path).read()
    kernels, meta = _kernels(asm)
    assert len(kernels) == 12, sorted(kernels)                                                  # {u8, f32, grid} x {NCHW, NHWC} x {aligned, not}
    for name, body in kernels.items():
        md = meta[name]
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", md).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s*(\d+)", md).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", md).group(1)) == 0, name
        assert int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", md).group(1)) == 0, name   # no LDS either
    bulk = {k: v for k, v in kernels.items() if re.search(r"export_(u8|grid)_kernelILi1ELb1E", k)}
    assert len(bulk) == 2, sorted(kernels)
    for name, body in bulk.items():
        mem = [x.split()[0] for x in body if re.match(r"(global|flat|buffer|scratch)_", x)]
        loads = [x for x in mem if "load" in x]
        stores = [x for x in mem if "store" in x]
        wide = [x for x in stores if not re.search(r"_(byte|short)", x)]
        assert set(loads) == {"global_load_dwordx4"}, (name, sorted(set(loads)))
        assert wide and set(wide) == {"global_store_dwordx4"}, (name, sorted(set(stores)))
        assert len(wide) == (8 if "u8" in name else 1), (name, len(wide))                       # 3 rgb + 1 mask + 4 rgba chunks; one chunk of a sheet
    nchw = [v for k, v in kernels.items() if re.search(r"export_(u8|grid)_kernelILi0ELb1E", k)]
    assert len(nchw) == 2
    for body in nchw:                                                                           # planes read in place, the same 16-byte stores
        assert any(x.startswith("global_store_dwordx4") for x in body)
