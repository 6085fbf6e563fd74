"""Host side of the Poisson blend (3d-magic-mirror_amd/poisson.py, csrc/mm_poisson.hip), no GPU.

This file holds the RESTATEMENT: the kernel's pipeline in elementwise torch operations on the CPU, fp32, one rounding per operation, in
the kernel's order -- the background path of test_pyramid_host.py's level 0, the right-hand side, and the red-black SOR sweeps on whole
planes.  tests/test_gpu_poisson.py holds the device to it with torch.equal.  Here the restatement is held to an fp64 sparse direct solve
of the same system, and that direct solve to the reference's own outputs (tests/golden/poisson_edit.npz, minted by
tests/golden/make_golden_poisson.py from poisson_image_editing.py with offset (0, 0))."""
import functools
import importlib
import os

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from test_composite_host import images, reflect_index, resize_restated
from test_export_host import as_float, quantize
from test_pyramid_host import pyramid_frames_restated

P = importlib.import_module("3d-magic-mirror_amd.poisson")

FAULTS = ("edge_value", "border_pinned", "odd_first", "b_border_from_source", "b_counts_outside")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def edge_cells(H, W):
    e = torch.zeros((H, W), dtype=torch.bool)
    e[0], e[-1], e[:, 0], e[:, -1] = True, True, True, True
    return e


def free_cells(inside, border, fault=None):
    """(...,H,W) bool: the cells that are solved for; the others are pinned to t"""
    if border == "pinned" or fault == "border_pinned":
        return inside.clone()
    return inside | edge_cells(*inside.shape[-2:])


def neighbours(v, mode="constant"):
    """left, right, up, down of every cell of (...,H,W); a neighbour outside the image is 0 (mode replicate: the faults' edge value)"""
    if mode == "replicate":
        H, W = v.shape[-2:]
        z = v[..., torch.arange(-1, H + 1).clamp(0, H - 1), :][..., torch.arange(-1, W + 1).clamp(0, W - 1)]
    else:
        z = F.pad(v, (1, 1, 1, 1))
    return z[..., 1:-1, :-2], z[..., 1:-1, 2:], z[..., :-2, 1:-1], z[..., 2:, 1:-1]


def rhs_restated(s, t, inside, fault=None):
    """b: fl(fl(4 s) - fl(fl(l + r) + fl(u + d))) inside the mask, t outside"""
    l, r, u, d = neighbours(s, "replicate" if fault == "b_counts_outside" else "constant")
    lap = 4.0 * s - ((l + r) + (u + d))
    return lap.expand(inside.shape).clone() if fault == "b_border_from_source" else torch.where(inside, lap, t)


def sor_restated(s, t, inside, border, sweeps, omega, fault=None):
    """(...,H,W) float32: x = t, then `sweeps` red-black sweeps, (y + x) even first; s, t (H,W) or (...,H,W), inside (...,H,W) bool"""
    H, W = inside.shape[-2:]
    free = free_cells(inside, border, fault)
    b = rhs_restated(s.float(), t.float(), inside, fault)
    x = t.float().expand(inside.shape).clone()
    om = torch.tensor(omega, dtype=torch.float32)
    even = (torch.arange(H)[:, None] + torch.arange(W)[None]) % 2 == 0
    colours = (~even, even) if fault == "odd_first" else (even, ~even)
    for _ in range(sweeps):
        for colour in colours:
            l, r, u, d = neighbours(x, "replicate" if fault == "edge_value" else "constant")
            new = x + om * (((b + ((l + r) + (u + d))) * 0.25) - x)
            x = torch.where(free & colour, new, x)
    return x


def poisson_float_restated(renders, backgrounds, low, mask=None):
    """(B,3,H,W) float32: the iterate before the quantiser.  renders (n_fg,4,H,W), backgrounds (n_bg,3|4,H,W), mask (n_fg,H,W) or None"""
    H, W = low["H"], low["W"]
    l, r, t, b = low["bg_pad"]
    ys, xs = reflect_index(torch.arange(H + t + b) - t, H), reflect_index(torch.arange(W + l + r) - l, W)
    out = []
    for o in range(low["B"]):
        fi = int(low["fg_index"][o])
        fg, bg = renders[fi], backgrounds[int(low["bg_index"][o])]
        inside = (quantize(fg[3]) != 0) if mask is None else (mask[fi] != 0)
        tgt = torch.stack([resize_restated(bg[c][ys][:, xs], 0, low["bg_y"], low["bg_x"]) for c in range(3)])
        out.append(sor_restated(fg[:3], tgt, inside[None].expand(3, H, W), low["border"], low["sweeps"], low["omega"]))
    return torch.stack(out)


def poisson_frames_restated(renders, backgrounds, bg_index, *, fg_index=None, mask=None, bg_pad=16, antialias=False, border="reference",
                            sweeps=None, omega=None, rounding="trunc", as_float_=False):
    """``poisson_frames`` on CPU tensors: (...,H,W,3) uint8 or (...,3,H,W) float32"""
    H, W = renders.shape[-2:]
    flat = renders.reshape((-1,) + tuple(renders.shape[-3:])).float()
    low = P.lower_poisson(H, W, flat.shape[0], backgrounds.shape[0], bg_index, fg_index, bg_pad=bg_pad, antialias=antialias, border=border,
                          sweeps=sweeps, omega=omega)
    q = quantize(poisson_float_restated(flat, backgrounds.float(), low, None if mask is None else mask.reshape(-1, H, W)), rounding)
    shape = tuple(np.shape(bg_index))
    return as_float(q).reshape(shape + (3, H, W)) if as_float_ else q.permute(0, 2, 3, 1).reshape(shape + (H, W, 3)).contiguous()


# ---- the same system, solved directly in fp64 ------------------------------------------------------------------------------------------
def direct_solve64(s, t, inside, border):
    """(H,W) float64: the restated system by a sparse direct solve.  s, t (H,W) float64, inside (H,W) bool (numpy)"""
    H, W = inside.shape
    free = free_cells(torch.from_numpy(inside), border).numpy()
    idx = np.arange(H * W).reshape(H, W)
    z = np.pad(s, 1)
    lap = 4.0 * s - (z[1:-1, :-2] + z[1:-1, 2:] + z[:-2, 1:-1] + z[2:, 1:-1])
    b = np.where(free, np.where(inside, lap, t), t)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.where(free, 4.0, 1.0).ravel()]
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        ok = free.copy()                                       # a neighbour inside the image; a missing one contributes nothing
        ok[:max(-dy, 0)] = False; ok[H - max(dy, 0):] = False; ok[:, :max(-dx, 0)] = False; ok[:, W - max(dx, 0):] = False
        rows.append(idx[ok]); cols.append(idx[ok] + dy * W + dx); vals.append(np.full(int(ok.sum()), -1.0))
    A = scipy.sparse.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W))
    return np.asarray(scipy.sparse.linalg.spsolve(A, b.ravel())).reshape(H, W)


# ---- 1. the direct solve against the reference's own outputs ---------------------------------------------------------------------------
def test_direct_solve_reproduces_the_references_bytes():
    """poisson_image_editing.py's outputs for 3x3, 9x7, 16x12 and 24x16 with interior, border-touching, all-zero and all-one masks: the
    outer-border rows (a Laplacian row against the target value) and the halved corners are the reference's, byte for byte."""
    z = np.load(os.path.join(GOLDEN, "poisson_edit.npz"))
    keys = sorted(k[len("result_"):] for k in z.files if k.startswith("result_"))
    assert len(keys) == 16
    close, corner = 0, []
    for key in keys:
        src, tgt, mask, want = (z[n + "_" + key] for n in ("source", "target", "mask", "result"))
        for c in range(3):
            x = direct_solve64(src[..., c].astype(np.float64), tgt[..., c].astype(np.float64), mask != 0, "reference")
            got = np.clip(x, 0.0, 255.0).astype(np.uint8)
            near = np.abs(x - np.round(x)) <= 1e-6
            close += int(near.sum())
            w = want[..., c].astype(np.int64)
            assert bool(((got == w) | (near & (np.abs(got.astype(np.int64) - w) <= 1))).all()), (key, c)
            if key.endswith("_zero") and tgt[0, 0, c] > 100:
                corner.append(float(x[0, 0]) / float(tgt[0, 0, c]))
    print("values within 1e-6 of an integer: %d; corner / target outside the mask: %.3f .. %.3f" % (close, min(corner), max(corner)))
    assert 0.3 < sum(corner) / len(corner) < 0.7               # a corner outside the mask comes out at about half its target


# ---- 2. / 3. the fp32 SOR restatement with the default sweeps and omega against the direct solve ---------------------------------------
SHAPES = ((1, 1), (2, 3), (3, 3), (8, 8), (16, 12), (31, 18), (64, 48), (128, 64), (128, 128), (160, 96))
MASKS = ("ellipse", "border", "ones", "zeros", "speckle")
BORDERS = ("reference", "pinned")


def make_mask(kind, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.arange(H)[:, None].float(), torch.arange(W)[None].float()
    if kind == "ellipse":
        return ((yy - (H - 1) / 2) / max(0.35 * H, 0.6)) ** 2 + ((xx - (W - 1) / 2) / max(0.3 * W, 0.6)) ** 2 <= 1.0
    if kind == "border":                                       # touches all four edges
        return (((yy - (H - 1) / 2) / (0.3 * H + 0.5)) ** 2 <= 1.0) | (((xx - (W - 1) / 2) / (0.2 * W + 0.5)) ** 2 <= 1.0)
    if kind == "ones":
        return torch.ones((H, W), dtype=torch.bool)
    if kind == "zeros":
        return torch.zeros((H, W), dtype=torch.bool)
    return torch.rand((H, W), generator=g) < 0.5


@functools.lru_cache(maxsize=None)
def grid(shape, fault=None, sweeps=None):
    """every mask x border of a shape, solved at once: the planes, the fp32 SOR iterate (with the call's default sweeps and omega unless
    `sweeps` is given) and, without a fault, the fp64 direct solve.  Computed once per shape and shared by the tests below; read only."""
    H, W = shape
    g = torch.Generator().manual_seed(100 * H + W)
    s, t = torch.rand((H, W), generator=g), torch.rand((H, W), generator=g)
    cases = [(m, b) for m in MASKS for b in BORDERS]
    masks = {m: make_mask(m, H, W, H + W) for m in MASKS}
    got = {}
    for b in BORDERS:                                          # the masks of one border mode are solved as one stack of planes
        inside = torch.stack([masks[m] for m in MASKS])
        x = sor_restated(s, t, inside, b, P.default_sweeps(H, W) if sweeps is None else sweeps, P.default_omega(H, W), fault)
        got.update({(m, b): x[i] for i, m in enumerate(MASKS)})
    want = None if fault else {(m, b): torch.from_numpy(direct_solve64(s.double().numpy(), t.double().numpy(), masks[m].numpy(), b)) for m, b in cases}
    return cases, got, want


@pytest.mark.parametrize("shape", SHAPES)
def test_default_sweeps_and_omega_reach_the_direct_solve(shape):
    """|fp32 SOR restatement - fp64 direct solve| with sweeps = max(4 N, 32) and omega = 2 / (1 + sin(pi / (N + 1))), N = max(H, W), over
    the masks ellipse, border-touching, all ones, all zeros and 50 % speckle and both borders.  The bar is the 1e-5 that the composite and
    pyramid restatements are held to.  Measured maxima on the CPU (profiles/poisson_kernels.md has the table): 1x1 0; 2x3 4.0e-8;
    3x3 8.9e-8; 8x8 1.9e-7; 16x12 3.3e-7; 31x18 5.0e-7; 64x48 1.1e-6; 128x64 2.2e-6; 128x128 2.3e-6; 160x96 2.7e-6 (at most 10 of
    153 600 bytes differ, each by one).
    The bytes differ from the direct solve's by at most one, and only where x * 255 lies within 2.6e-3 (255 x the bar) of an integer."""
    cases, got, want = grid(shape)
    worst, off, lo, hi = 0.0, 0, 0.0, 1.0
    for case in cases:
        x, w = got[case], want[case]
        err = float((x.double() - w).abs().max())
        worst, lo, hi = max(worst, err), min(lo, float(w.min())), max(hi, float(w.max()))
        assert err <= 1e-5, (shape, case, err)
        q, q64 = quantize(x).long(), (w * 255).clamp(0, 255).floor().long()
        near = ((w * 255) - (w * 255).round()).abs() <= 2.6e-3
        assert bool(((q == q64) | (near & ((q - q64).abs() <= 1))).all()), (shape, case)
        off += int((q != q64).sum())
    print("%s: max |fp32 SOR - fp64 direct| = %.3g over %d cases; %d of %d bytes differ; the solution ranges over %.3f .. %.3f"
          % (shape, worst, len(cases), off, len(cases) * shape[0] * shape[1], lo, hi))
    assert off <= 0.01 * len(cases) * shape[0] * shape[1]


# ---- 4. the cases catch a restatement that is wrong -------------------------------------------------------------------------------------
FAULT_SHAPES = ((2, 3), (3, 3), (9, 7), (16, 12), (31, 18))


@pytest.mark.parametrize("fault", FAULTS)
def test_cases_catch_each_fault(fault):
    """A copy of the restatement with one fault switched on misses the checks above (on the shapes up to 31 x 18, which keep this quick).
    Four of the faults change the system and leave the converged iterate more than 1e-5 from the direct solve; the fifth, the colours
    swept in the other order, converges to the same solution and is what the 8-sweep cases of tests/test_gpu_poisson.py hold with
    torch.equal: the iterate after 8 sweeps differs, and so do its bytes."""
    caught = []
    for shape in FAULT_SHAPES:
        cases, good, want = grid(shape)
        if fault == "odd_first":
            _, bad8, _ = grid(shape, fault, 8)
            _, good8, _ = grid(shape, None, 8)
            caught += [(shape, c) for c in cases if not torch.equal(quantize(bad8[c]), quantize(good8[c]))]
        else:
            _, bad, _ = grid(shape, fault)
            caught += [(shape, c) for c in cases if float((bad[c].double() - want[c]).abs().max()) > 1e-5]
        assert all(float((good[c].double() - want[c]).abs().max()) <= 1e-5 for c in cases)
    print(fault, "caught by %d of %d cases" % (len(caught), len(FAULT_SHAPES) * len(MASKS) * len(BORDERS)))
    assert caught, fault
    if fault in ("border_pinned", "b_border_from_source"):    # (only the reference's border has free cells outside the mask)
        assert all(c[1] == "reference" for _, c in caught)


def test_one_sweep_by_hand():
    """1 x 2, all inside, omega 1: the even cell first, from the odd cell's OLD value; then the odd cell from the even cell's NEW one"""
    s, t = torch.tensor([[0.75, 0.25]]), torch.tensor([[0.5, 0.125]])
    x = sor_restated(s, t, torch.ones((1, 2), dtype=torch.bool), "reference", 1, 1.0)
    b0, b1 = 4 * 0.75 - 0.25, 4 * 0.25 - 0.75
    x0 = (b0 + 0.125) * 0.25
    x1 = (b1 + x0) * 0.25
    assert x.tolist() == [[x0, x1]]                            # (every value is a dyadic rational: exact in fp32)
    y = sor_restated(s, t, torch.ones((1, 2), dtype=torch.bool), "reference", 1, 1.0, fault="odd_first")
    assert y.tolist() == [[(b0 + (b1 + 0.5) * 0.25) * 0.25, (b1 + 0.5) * 0.25]]


def test_target_is_the_pyramids_level_zero_background():
    """all-zero mask, every cell pinned: the frames are the quantised background path, which a pyramid of one-tap blurs also gives"""
    x, bg = images(3, 2, 4, 24, 18, 5)
    x[:, 3] = 0
    for aa in (False, True):
        kw = dict(bg_pad=(3, 5, 8, 2), antialias=aa)
        got = poisson_frames_restated(x, bg, [1, 0, 1], border="pinned", **kw)
        assert torch.equal(got, pyramid_frames_restated(x, bg, [1, 0, 1], blur=torch.ones(1), **kw))


# ---- 5. lowering and errors ---------------------------------------------------------------------------------------------------------
def test_wrapper_validates_before_anything_reaches_a_kernel():
    x, bg = images(3, 2, 4, 16, 12, 1)
    idx = [1, 0, 1]
    ok_mask = torch.ones((3, 16, 12), dtype=torch.bool)
    for kw, what in ((dict(mask=torch.ones((3, 12, 16), dtype=torch.bool)), "mask must have"), (dict(mask=torch.ones((2, 16, 12), dtype=torch.uint8)), "mask must have"),
                     (dict(mask=torch.ones((3, 16, 12))), "bool or uint8"), (dict(border="free"), "border"), (dict(rounding="floor"), "rounding"),
                     (dict(sweeps=-1), "sweeps"), (dict(omega=0.0), "omega"), (dict(omega=2.0), "omega"), (dict(omega=-0.5), "omega"),
                     (dict(omega=float("nan")), "omega"), (dict(bg_pad=12), "reflection pad"), (dict(bg_pad=(-1, 0, 0, 0)), "negative"),
                     (dict(fg_index=[0, 1, 3]), "fg_index outside"), (dict(fg_index=[0, 1]), "bg_index must have")):
        with pytest.raises(ValueError, match=what):
            P.poisson_frames(x, bg, idx, **dict(dict(mask=ok_mask, bg_pad=4), **kw))
    for bad in ([0, 1, 2], [0, -1, 1]):
        with pytest.raises(ValueError, match="bg_index outside"):
            P.poisson_frames(x, bg, bad, bg_pad=4)
    with pytest.raises(RuntimeError, match="device memory"):   # valid, on the CPU: refused by the launch, after the lowering
        P.poisson_frames(x, bg, idx, bg_pad=4)
    before = x.clone()
    low = P.lower_poisson(16, 12, 3, 2, torch.tensor(idx), bg_pad=4)
    assert torch.equal(x, before) and low["B"] == 3 and low["border"] == "reference"
    assert low["sweeps"] == 64 and low["omega"] == float(np.float32(2.0 / (1.0 + np.sin(np.pi / 17.0))))
    assert low["params"].dtype == torch.int32 and low["params"].numel() == 6 + 10 * (16 + 12)
    assert P.lower_poisson(3, 5, 1, 1, [0], bg_pad=0)["sweeps"] == 32 and P.lower_poisson(3, 5, 1, 1, [0], bg_pad=0, sweeps=0)["sweeps"] == 0
    assert P.PRESETS["tool/generate_market_test"] == dict(bg_pad=16)


def largest_square(bg_pad=16):
    """the largest n for which an n x n call fits the LDS (the planes grow with n: the first refusal ends the search)"""
    n = 128
    while True:
        try:
            P.lower_poisson(n + 1, n + 1, 1, 1, [0], bg_pad=bg_pad)
        except ValueError:
            return n
        n += 1


def test_lds_bytes_by_hand_and_the_refusal():
    """two colour planes of (H + 2) x ((W + 3) // 2) words and the staging rows of the vertical resize: behind a pad of 16 a band of 8
    output rows reads 10 padded rows at both shapes (160 -> 128 steps by 1.25 from 0.125: rows 10 k .. 10 k + 9)"""
    low = P.lower_poisson(128, 64, 1, 1, [0])
    assert low["lds_bytes"] == P.lds_bytes(low) == 4 * (2 * 4292 + 10 * 64) == 36896          # (130 * 33 = 4290, rounded up to 4 floats)
    low = P.lower_poisson(128, 128, 1, 1, [0])
    assert low["lds_bytes"] == 4 * (2 * 8452 + 10 * 128) == 72736 > 64 * 1024                # (130 * 65 = 8450): the first plane past 64 KiB
    assert P.lower_poisson(128, 128, 1, 1, [0], bg_pad=0)["lds_bytes"] == 4 * (2 * 8452 + 8 * 128)
    with pytest.raises(ValueError, match=r"takes 275488 bytes of LDS, more than 163840"):   # 4 * (2 * 33284 + 9 * 256): 258 * 129 = 33282; 288 -> 256 reads 9 rows
        P.lower_poisson(256, 256, 1, 1, [0])
    n = largest_square()
    assert 128 < n < 256 and P.lower_poisson(n, n, 1, 1, [0])["lds_bytes"] <= 160 * 1024
    with pytest.raises(ValueError, match="LDS"):
        P.lower_poisson(n + 1, n + 1, 1, 1, [0])


def test_c_abi_refuses_before_any_gpu_work():
    N = importlib.import_module("3d-magic-mirror_amd._native")
    import ctypes
    lib = N.lib()
    assert lib.mm_struct_size(40) == ctypes.sizeof(N.MMPoissonDesc) > 0
    assert lib.mm_poisson_frames(None, None) == -1
    low = P.lower_poisson(16, 12, 3, 2, [1, 0, 1], bg_pad=4)
    par = low["params"].clone()
    d = N.MMPoissonDesc()
    d.B, d.H, d.W, d.n_fg, d.n_bg, d.bg_C = 3, 16, 12, 3, 2, 3
    d.bg_pad = (ctypes.c_int32 * 4)(4, 4, 4, 4)
    d.sweeps, d.omega = 8, 1.5
    one = ctypes.c_void_p(par.data_ptr())                      # (never dereferenced as device memory: every call below is refused first)
    d.renders = d.backgrounds = d.params = d.out = one
    assert lib.mm_poisson_frames(ctypes.byref(d), None) == -1   # params_host is NULL
    d.params_host = one
    for field, bad in (("border", 2), ("rounding", 2), ("sweeps", -1), ("sweeps", N.POISSON_MAX_SWEEPS + 1), ("omega", 0.0), ("omega", 2.0),
                       ("omega", float("nan")), ("bg_C", 2), ("n_bg", 1), ("W", 0)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        assert lib.mm_poisson_frames(ctypes.byref(d), None) == -2, field
        setattr(d, field, keep)
    par[6 + 1] = 9                                             # a resize row with nine taps
    assert lib.mm_poisson_frames(ctypes.byref(d), None) == -2
    rows = [P._rows(P.resize_taps(288, 256)).reshape(-1)] * 2  # valid tables of a plane that does not fit
    par2 = torch.from_numpy(np.concatenate([np.zeros(2, dtype=np.int32)] + rows))
    d.B, d.H, d.W, d.n_fg, d.n_bg = 1, 256, 256, 1, 1
    d.bg_pad = (ctypes.c_int32 * 4)(16, 16, 16, 16)
    d.params_host = ctypes.c_void_p(par2.data_ptr())
    assert lib.mm_poisson_frames(ctypes.byref(d), None) == -5   # MM_ERR_UNSUPPORTED


# ---- 6. the kernel's metadata ----------------------------------------------------------------------------------------------------------
def test_kernel_uses_no_scratch_no_spill_and_no_static_lds():
    """resources only, read from the metadata of the compiled kernel, for every instance (slots per lane): no scratch, no vector-register
    spill -- the cells' b and x live in registers --, no static LDS in front of the dynamic region, workgroups of 1024"""
    import re
    import subprocess
    import tempfile
    bn = importlib.import_module("3d-magic-mirror_amd.build_native")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert bn.SOURCES["mm_poisson.hip"] == bn.EXACT
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "poisson.s")
        subprocess.check_call([hipcc] + bn.FLAGS + bn.SOURCES["mm_poisson.hip"] + ["-S", "--cuda-device-only", "-o", path,
                                                                                    os.path.join(bn.CSRC, "mm_poisson.hip")], stderr=subprocess.DEVNULL)
        asm = open(path).read()
    names = re.findall(r"^(_ZN2mm\w*poisson_kernel\w*):", asm, flags=re.M)
    assert len(names) == 7, names
    for name in names:
        meta = [e for e in re.split(r"\n  - (?=\.)", asm[asm.index("amdhsa.kernels:"):]) if re.search(r"\.name:\s+%s$" % re.escape(name), e, flags=re.M)][0]
        for key in ("private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size"):
            assert int(re.search(r"\.%s:\s*(\d+)" % key, meta).group(1)) == 0, (name, key)
        assert int(re.search(r"\.max_flat_workgroup_size:\s*(\d+)", meta).group(1)) == 1024
        assert int(re.search(r"\.vgpr_count:\s*(\d+)", meta).group(1)) <= 128
