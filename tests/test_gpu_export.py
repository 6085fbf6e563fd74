"""Export of renders to 8-bit frames and contact sheets on the MI355X (csrc/mm_export.hip) against the eager torch restatement evaluated
on the CPU (tests/test_export_host.py), with torch.equal: every operation is one correctly rounded fp32 multiply, add, subtract or
divide, or an exact conversion, and the file is compiled without contraction, so there is no tolerance to measure.

Shapes are the smallest that reach each path: (3,4,5,7) has 105 rgb bytes per image, so images start at every byte alignment, 16-pixel
groups span images and 9 pixels are left for the byte path; (2,4,8,8) is whole groups only; (1,4,1,1) the byte path only.  The sheets
are 5x7 cells throughout: 105 bytes per cell line, so chunks span rows, cells and frames, and all but the 16x74 sheet (3552 bytes) have
a tail."""
import importlib
import itertools
import os

import pytest
import torch

from conftest import TEMPLATES
from test_export_host import export_grid_restated, export_images_restated

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EX = importlib.import_module("3d-magic-mirror_amd.export")
CHANNELS = ("rgb", "mask", "rgba", "rgb+mask")


def values(shape, seed):
    """a CPU tensor of `shape` = (...,C,H,W) in NCHW memory: uniform in [-0.5, 1.5], then -- spread over the whole tensor -- every k/255
    with its two fp32 neighbours (as far as they fit), 0, 1, -0.0, NaN and +-inf; a 4th channel is an alpha with exact 0s and 1s"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g) * 2 - 0.5
    if shape[-3] == 4:
        a = torch.rand(shape[:-3] + shape[-2:], generator=g) * 2 - 0.5
        x[..., 3, :, :] = a.clamp(0, 1)                                                         # a quarter exact 0, a quarter exact 1
    k = torch.arange(256, dtype=torch.float32) / torch.full((256,), 255.0)
    triples = torch.stack((k, torch.nextafter(k, torch.tensor(2.0)), torch.nextafter(k, torch.tensor(-2.0))), 1)
    special = torch.cat((torch.tensor([0.0, 1.0, -0.0, float("nan"), float("inf"), -float("inf")]),
                         triples[torch.randperm(256, generator=g)].reshape(-1)))      # a small tensor takes a seeded choice of the k
    flat = x.reshape(-1)
    n = min(special.numel(), max(1, flat.numel() // 2))
    where = torch.randperm(flat.numel(), generator=g)[:n]
    flat[where] = special[:n]
    return x


def layout(x, nhwc):
    """the same values in the memory the flag names (NHWC: (...,H,W,C) memory seen as (...,C,H,W))"""
    return x.movedim(-3, -1).contiguous().movedim(-1, -3) if nhwc else x.contiguous()


def to_dev(x):
    """the same values with the same strides in device memory"""
    d = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=DEV)
    d.copy_(x)
    return d


def same(got, want, what):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.is_contiguous() and a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, tuple(a.shape), tuple(b.shape))
        assert torch.equal(a.cpu(), b), what


def check_images(x, nhwc):
    xd = to_dev(layout(x, nhwc))
    C = x.shape[-3]
    for rounding, wh, ch, fl in itertools.product(("trunc", "nearest"), (False, True), CHANNELS, (False, True)):
        if C == 3 and (wh or ch != "rgb"):
            continue
        got = EX.export_images(xd, ch, rounding=rounding, white=wh, as_float=fl)
        same(got, export_images_restated(x, ch, rounding, wh, fl), (tuple(x.shape), nhwc, rounding, wh, ch, fl))


@pytest.mark.parametrize("nhwc", (0, 1))
@pytest.mark.parametrize("shape", ((3, 4, 5, 7), (2, 4, 8, 8), (1, 4, 1, 1), (2, 3, 4, 5, 7)))
def test_images(pkg, shape, nhwc):
    check_images(values(shape, 11 + len(shape) + shape[-1]), nhwc)


def test_three_channel_images(pkg):
    check_images(values((2, 3, 5, 7), 5), 0)
    x = values((2, 3, 5, 7), 6)
    same(EX.export_images(to_dev(layout(x, 1))), export_images_restated(x), "12-byte pixels go through the copy")


def test_plane_groups_of_sixteen(pkg):
    """H*W a multiple of 16 with more than one workgroup: the NCHW path that reads a group as four 16-byte loads per plane"""
    x = values((3, 4, 48, 48), 9)
    for nhwc in (0, 1):
        xd = to_dev(layout(x, nhwc))
        same(EX.export_images(xd, "rgb+mask", white=True), export_images_restated(x, "rgb+mask", "trunc", True), nhwc)
        same(EX.export_images(xd, "rgba", rounding="nearest"), export_images_restated(x, "rgba", "nearest"), nhwc)


GRIDS = [  # B, N (None: a 4-D batch), nrow, padding, pad_value
    (1, None, 8, 2, 0.0), (1, 3, 8, 2, 1.0), (3, None, 8, 2, 0.5), (3, 3, 8, 0, 0.0), (9, 1, 8, 2, 1.0), (9, 3, 8, 2, 0.5),
    (9, None, 3, 2, 0.0), (9, 3, 3, 0, 0.5), (9, 3, 8, 0, 1.0), (3, 1, 1, 2, 0.0)]


@pytest.mark.parametrize("nhwc", (0, 1))
@pytest.mark.parametrize("B,Nv,nrow,padding,pad_value", GRIDS)
def test_grids(pkg, B, Nv, nrow, padding, pad_value, nhwc):
    x = values((B, 4, 5, 7) if Nv is None else (B, Nv, 4, 5, 7), 100 + B + nrow)
    xd = to_dev(layout(x, nhwc))
    for rounding in ("trunc", "nearest"):
        got = EX.export_grid(xd, nrow=nrow, padding=padding, pad_value=pad_value, rounding=rounding)
        want = export_grid_restated(x, nrow, padding, pad_value, rounding)
        same(got, want, (B, Nv, nrow, padding, pad_value, nhwc, rounding))


def test_grid_over_white_three_channels_and_many_chunks(pkg):
    x = values((9, 3, 4, 5, 7), 42)
    for nhwc in (0, 1):
        same(EX.export_grid(to_dev(layout(x, nhwc)), white=True, pad_value=1.0), export_grid_restated(x, pad_value=1.0, white_=True), nhwc)
    x3 = values((3, 2, 3, 5, 7), 43)
    same(EX.export_grid(to_dev(x3), rounding="nearest"), export_grid_restated(x3, rounding="nearest"), "C = 3")
    big = values((20, 2, 4, 40, 24), 44)                                                        # more than one workgroup of chunks
    same(EX.export_grid(to_dev(layout(big, 1)), nrow=6), export_grid_restated(big, nrow=6), "3 x 6 cells of 40 x 24")


def test_strided_and_float64_inputs_go_through_the_copy(pkg):
    x = values((3, 4, 5, 14), 7)
    xd = to_dev(x)
    same(EX.export_images(xd[..., ::2], "rgb+mask"), export_images_restated(x[..., ::2], "rgb+mask"), "strided images")
    same(EX.export_grid(xd[..., ::2]), export_grid_restated(x[..., ::2]), "strided grid")
    same(EX.export_images(xd[1:, :3]), export_images_restated(x[1:, :3]), "a channel slice")
    x64 = values((3, 4, 5, 7), 8).double() + 1e-12
    for nhwc in (0, 1):
        xd = to_dev(layout(x64, nhwc))
        same(EX.export_images(xd, "rgba", rounding="nearest"), EX.export_images(xd.float(), "rgba", rounding="nearest").cpu(), "float64 images")
        same(EX.export_images(xd, "rgba"), export_images_restated(x64.float(), "rgba"), "float64 images")
        same(EX.export_grid(xd), export_grid_restated(x64.float()), "float64 grid")


def test_end_to_end_from_render_views(pkg):
    B, n, S = 2, 3, 32
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), S)
    att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, B, S, S, seed=0)
    a = {k: att[k].to(DEV) for k in ("vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases")}
    a["azimuths"] = (a["azimuths"][:, None] + torch.arange(n, device=DEV, dtype=torch.float32)[None] * 120.0).contiguous()
    with torch.no_grad():
        frames, _ = dr.render_views(no_mask=False, **a)
    assert frames.shape == (B, n, 4, S, S) and not frames.is_contiguous() and EX._layout(frames)[1] == 1
    before = frames.clone()
    host = frames.cpu()
    sheet = EX.export_grid(frames)
    assert sheet.shape == (n,) + EX.grid_shape(B, S, S) + (3,)
    same(sheet, export_grid_restated(host), "turntable sheets")
    rgb, mask = EX.export_images(frames, "rgb+mask")
    want = export_images_restated(host, "rgb+mask")
    assert rgb.shape == (B, n, S, S, 3) and mask.shape == (B, n, S, S)
    for b in range(B):
        for v in range(n):
            assert torch.equal(rgb[b, v].cpu(), want[0][b, v]) and torch.equal(mask[b, v].cpu(), want[1][b, v]), (b, v)
    assert 0 < int(mask.count_nonzero()) < mask.numel()                                          # the sphere covers part of the image
    same(EX.export_images(frames, "rgb", white=True, as_float=True), export_images_restated(host, "rgb", white_=True, float_=True), "scored form")
    assert torch.equal(frames, before)


def test_two_runs_give_the_same_bytes(pkg):
    xd = to_dev(layout(values((9, 3, 4, 5, 7), 77), 1))
    assert torch.equal(EX.export_grid(xd, rounding="nearest"), EX.export_grid(xd, rounding="nearest"))
    a, b = EX.export_images(xd, "rgb+mask"), EX.export_images(xd, "rgb+mask")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

