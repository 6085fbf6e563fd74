"""The composite of renders over blurred backgrounds on the MI355X (csrc/mm_composite.hip) against the eager torch restatement evaluated
on the CPU (tests/test_composite_host.py), with torch.equal: every operation is one correctly rounded fp32 multiply, add, subtract or
divide, an exact conversion, or a table value from the host, and the file is compiled without contraction, so there is no tolerance to
measure.

Shapes are the smallest that reach each path.  5 x 7 is one band of 105 bytes per frame, so frames start at every byte alignment and the
bytes before and after the aligned chunks are all exercised; 24 x 18 with pad (8,8,16,16) and kernel 31 has a halo wider than the image
(indices reflected twice); 37 x 41 is four bands of MM_COMPOSITE_ROWS = 8 rows and a remainder of 5 (rows are the only tiled axis), with
984 bytes per band and 4551 per frame, so bands start at both phases of 8 bytes; 16 x 16 is whole bands and whole 16-byte chunks only."""
import importlib
import itertools
import os

import pytest
import torch

from conftest import TEMPLATES
from test_composite_host import composite_frames_restated
from test_gpu_export import layout, to_dev

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
C = importlib.import_module("3d-magic-mirror_amd.composite")


def values(lead, n_bg, bg_C, H, W, seed):
    """CPU renders lead + (4,H,W) and backgrounds (n_bg,bg_C,H,W): rgb and backgrounds uniform in [0, 1]; a mask with exact 0s and 1s
    (a quarter each) and soft values between; then, spread over the rgb planes, a few k/255 with their two fp32 neighbours, and in the
    first render one NaN and one inf pixel (where the image has room for them)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(tuple(lead) + (4, H, W), generator=g)
    x[..., 3, :, :] = (torch.rand(tuple(lead) + (H, W), generator=g) * 2 - 0.5).clamp(0, 1)
    k = torch.randint(0, 256, (8,), generator=g).float() / torch.full((8,), 255.0)
    special = torch.stack((k, torch.nextafter(k, torch.tensor(2.0)), torch.nextafter(k, torch.tensor(-2.0))), 1).reshape(-1)
    rgb = x[..., :3, :, :]
    n = min(special.numel(), rgb.numel() // 4)
    where = torch.randperm(rgb.numel(), generator=g)[:n]
    flat = rgb.reshape(-1)
    flat[where] = special[:n]
    x[..., :3, :, :] = flat.reshape(rgb.shape)
    first = x.reshape((-1, 4, H, W))[0]
    first[0, H // 2, W // 2] = float("nan")
    first[1, H - 1, 0] = float("inf")
    return x, torch.rand((n_bg, bg_C, H, W), generator=g)


def same(got, want, what):
    assert got.is_contiguous() and got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, tuple(got.shape), tuple(want.shape))
    assert torch.equal(got.cpu(), want), what


@pytest.mark.parametrize("bg_C", (3, 4))
@pytest.mark.parametrize("nhwc", (0, 1))
def test_small_frames_every_option(pkg, nhwc, bg_C):
    x, bg = values((3,), 2, bg_C, 5, 7, 3 + bg_C)
    xd, bgd = to_dev(layout(x, nhwc)), to_dev(bg)
    fgi, bgi = [2, 0, 2, 1], torch.tensor([1, 1, 0, 1])                                          # repeats, out of order
    sig_m, sig_b = torch.tensor([3.0, 0.4, 1.1, 2.0]), torch.tensor([0.1, 1.9, 0.7, 1.3])       # one sigma per frame and plane
    for fill, aa in itertools.product((False, True), (False, True)):
        kw = dict(fg_index=fgi, fill_holes=fill, mask_blur=(5, sig_m), mask_pad=3, bg_pad=(2, 3, 1, 2), bg_blur=(5, sig_b), antialias=aa)
        for rounding, fl in itertools.product(("trunc", "nearest"), (False, True)):
            got = C.composite_frames(xd, bgd, bgi, rounding=rounding, as_float=fl, **kw)
            assert got.shape == ((4, 3, 5, 7) if fl else (4, 5, 7, 3))
            same(got, composite_frames_restated(x, bg, bgi, rounding=rounding, as_float_=fl, **kw), (nhwc, bg_C, fill, aa, rounding, fl))


def test_stages_left_out(pkg):
    """no blur, no pad, no resize: the plain blend; and each stage alone"""
    x, bg = values((3,), 2, 3, 5, 7, 9)
    xd, bgd = to_dev(x), to_dev(bg)
    bgi = [0, 1, 1]
    for kw in (dict(), dict(fill_holes=True), dict(mask_blur=(3, 1.0)), dict(mask_pad=2), dict(bg_pad=(0, 2, 1, 0)), dict(bg_blur=(5, 0.8)),
               dict(bg_blur=torch.tensor([0.25, 0.5, 0.25]), antialias=True, bg_pad=1)):
        same(C.composite_frames(xd, bgd, bgi, **kw), composite_frames_restated(x, bg, bgi, **kw), kw)


@pytest.mark.parametrize("antialias", (False, True))
def test_halo_wider_than_the_image(pkg, antialias):
    x, bg = values((2,), 2, 3, 24, 18, 24)
    kw = dict(fill_holes=True, mask_blur=(31, 2.0), mask_pad=3, bg_pad=(8, 8, 16, 16), bg_blur=(31, 2.0), antialias=antialias)
    same(C.composite_frames(to_dev(layout(x, 1)), to_dev(bg), [1, 0], **kw), composite_frames_restated(x, bg, [1, 0], **kw), antialias)


@pytest.mark.parametrize("H,W", ((37, 41), (16, 16)))
def test_bands_and_remainders(pkg, H, W):
    x, bg = values((3,), 3, 4, H, W, H)
    bgi = [2, 0, 1]
    for nhwc, aa, fl in ((1, False, False), (0, True, False), (1, True, True)):
        kw = dict(fill_holes=True, mask_blur=(5, 3.0), mask_pad=3, bg_pad=(5, 4, 9, 7), bg_blur=(7, torch.tensor([0.3, 1.0, 1.9])), antialias=aa)
        got = C.composite_frames(to_dev(layout(x, nhwc)), to_dev(bg), bgi, as_float=fl, **kw)
        same(got, composite_frames_restated(x, bg, bgi, as_float_=fl, **kw), (H, W, nhwc, aa, fl))


@pytest.mark.parametrize("site", sorted(C.PRESETS))
def test_call_sites_at_the_market_shape(pkg, site):
    x, bg = values((4,), 4, 4, 128, 64, 128)
    kw = C.preset(site, 4, generator=torch.Generator().manual_seed(2))
    bgi = torch.tensor([3, 0, 0, 2])
    xd, bgd = to_dev(layout(x, 1)), to_dev(bg)
    before = xd.clone(), bgd.clone()
    got = C.composite_frames(xd, bgd, bgi, **kw)
    same(got, composite_frames_restated(x, bg, bgi, **kw), site)
    assert torch.equal(xd.view(torch.int32), before[0].view(torch.int32)) and torch.equal(bgd, before[1])   # the inputs are left alone (bits: x holds a NaN)
    assert torch.equal(C.composite_frames(xd, bgd, bgi, **kw), got)                              # and two runs give the same bytes
    host = got.cpu().numpy()
    assert host.shape == (4, 128, 64, 3) and host.dtype.name == "uint8"


def test_render_views_shaped_input(pkg):
    x, bg = values((2, 3), 2, 4, 8, 8, 8)
    bgi = torch.tensor([[1, 0, 1], [0, 0, 1]])
    kw = dict(fill_holes=True, mask_blur=(5, 3.0), mask_pad=3, bg_pad=(2, 2, 3, 3), bg_blur=(5, 1.2))
    for nhwc in (0, 1):
        got = C.composite_frames(to_dev(layout(x, nhwc)), to_dev(bg), bgi, **kw)
        assert got.shape == (2, 3, 8, 8, 3)
        same(got, composite_frames_restated(x, bg, bgi, **kw), nhwc)
    fgi = torch.tensor([[5, 0], [3, 3]])                                                         # flat over (B,N)
    got = C.composite_frames(to_dev(layout(x, 1)), to_dev(bg), bgi[:, :2], fg_index=fgi, as_float=True, **kw)
    assert got.shape == (2, 2, 3, 8, 8)
    same(got, composite_frames_restated(x, bg, bgi[:, :2], fg_index=fgi, as_float_=True, **kw), "fg_index")
    xd = to_dev(x)
    same(C.composite_frames(xd[..., ::2], to_dev(bg)[..., ::2], bgi, bg_pad=1), composite_frames_restated(x[..., ::2], bg[..., ::2], bgi, bg_pad=1), "strided")
    same(C.composite_frames(xd.double(), to_dev(bg).double(), bgi, **kw), composite_frames_restated(x, bg, bgi, **kw), "float64 goes through .float()")


def test_end_to_end_from_render(pkg):
    B, S = 2, 32
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), S)
    att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, B, S, S, seed=0)
    a = {k: att[k].to(DEV) for k in ("vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases")}
    with torch.no_grad():
        pred, _ = dr.render(no_mask=False, **a)
    assert pred.shape == (B, 4, S, S) and not pred.is_contiguous()
    Xa = gt.to(DEV)
    kw = C.preset("generate_market++", B, generator=torch.Generator().manual_seed(0))
    kw["bg_pad"] = (4, 4, 8, 8)
    frames = pkg.composite_frames(pred, Xa, [1, 0], **kw)
    same(frames, composite_frames_restated(pred.cpu(), gt, [1, 0], **kw), "render over the input batch")
    assert 0 < int((frames != 0).sum())
