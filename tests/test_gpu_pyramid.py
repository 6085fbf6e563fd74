"""The three-level pyramid blend on the MI355X (csrc/mm_pyramid.hip) against the eager torch restatement evaluated on the CPU
(tests/test_pyramid_host.py), with torch.equal: every operation is one correctly rounded fp32 multiply, add, subtract or divide, an exact
conversion, or a table value from the host, and the file is compiled without contraction, so there is no tolerance to measure.

Shapes are the smallest that reach each path.  5 x 7 with kernel 3 is one band shorter than MM_PYRAMID_ROWS = 8 and narrower than the
cascade's halo of 3 + 3, so both edges reflect inside one band, and its 105 bytes per frame start frames at every byte alignment; 37 x 41
with kernel 7 is four bands and a remainder of 5 whose halos of 9 rows are cut at the top, at the bottom, or not at all, with an odd width
and bands that start at both phases of 8 bytes; 16 x 16 is whole bands and whole 16-byte chunks, every band's halo cut at an edge;
24 x 18 with kernel 15 has a halo of 21 rows, wider than the image, so every band stages the whole image; 128 x 64 is the call site."""
import importlib

import pytest
import torch

from test_export_host import quantize
from test_gpu_composite import same, values
from test_gpu_export import layout, to_dev
from test_pyramid_host import pyramid_frames_restated

pytestmark = pytest.mark.gpu

P = importlib.import_module("3d-magic-mirror_amd.pyramid")
C = importlib.import_module("3d-magic-mirror_amd.composite")


def nine_sigmas(n, seed):
    """(n,3,3) distinct sigmas, so that a swapped frame, plane-kind or level index shows"""
    return C.draw_sigmas(9 * n, generator=torch.Generator().manual_seed(seed)).view(n, 3, 3)


@pytest.mark.parametrize("bg_C", (3, 4))
@pytest.mark.parametrize("nhwc", (0, 1))
def test_image_shorter_than_a_band_and_narrower_than_the_halo(pkg, nhwc, bg_C):
    x, bg = values((3,), 2, bg_C, 5, 7, 5 + bg_C)
    xd, bgd = to_dev(layout(x, nhwc)), to_dev(bg)
    fgi, bgi = [2, 0, 2, 1], torch.tensor([1, 1, 0, 1])                                          # repeats, out of order
    for aa in (False, True):
        kw = dict(fg_index=fgi, blur=(3, nine_sigmas(4, 1)), bg_pad=(2, 3, 1, 2), antialias=aa)
        for rounding, fl in (("trunc", False), ("nearest", False), ("nearest", True)):
            got = P.pyramid_frames(xd, bgd, bgi, rounding=rounding, as_float=fl, **kw)
            assert got.shape == ((4, 3, 5, 7) if fl else (4, 5, 7, 3))
            same(got, pyramid_frames_restated(x, bg, bgi, rounding=rounding, as_float_=fl, **kw), (nhwc, bg_C, aa, rounding, fl))


@pytest.mark.parametrize("H,W", ((37, 41), (16, 16)))
def test_bands_and_remainders(pkg, H, W):
    x, bg = values((3,), 3, 4, H, W, H)
    bgi = [2, 0, 1]
    sig = nine_sigmas(3, H)
    assert sig.unique().numel() == 27
    for nhwc, aa, fl in ((1, False, False), (0, True, True)):
        kw = dict(blur=(7, sig), bg_pad=(5, 4, 9, 7), antialias=aa)
        got = P.pyramid_frames(to_dev(layout(x, nhwc)), to_dev(bg), bgi, as_float=fl, **kw)
        same(got, pyramid_frames_restated(x, bg, bgi, as_float_=fl, **kw), (H, W, nhwc, aa, fl))
    taps = C.gaussian_taps(7, sig[0].reshape(-1)).reshape(3, 3, 7)                               # ready taps, shared by the frames
    same(P.pyramid_frames(to_dev(x), to_dev(bg), bgi, blur=taps, bg_pad=3), pyramid_frames_restated(x, bg, bgi, blur=taps, bg_pad=3), "ready taps")


def test_halo_wider_than_the_image(pkg):
    x, bg = values((2,), 2, 3, 24, 18, 24)
    kw = dict(blur=(15, nine_sigmas(2, 3) * 2), bg_pad=(8, 8, 16, 16))
    same(P.pyramid_frames(to_dev(layout(x, 1)), to_dev(bg), [1, 0], **kw), pyramid_frames_restated(x, bg, [1, 0], **kw), "kernel 15")


def test_call_site_at_the_market_shape(pkg):
    x, bg = values((4,), 4, 4, 128, 64, 128)
    kw = P.preset("tool/generate_market_test", 4, generator=torch.Generator().manual_seed(2))
    assert kw["bg_pad"] == 16 and kw["blur"][0] == 7
    bgi = torch.tensor([3, 0, 0, 2])
    xd, bgd = to_dev(layout(x, 1)), to_dev(bg)
    before = xd.clone(), bgd.clone()
    got = P.pyramid_frames(xd, bgd, bgi, **kw)
    same(got, pyramid_frames_restated(x, bg, bgi, **kw), "preset")
    assert torch.equal(xd.view(torch.int32), before[0].view(torch.int32)) and torch.equal(bgd, before[1])   # the inputs are left alone (bits: x holds a NaN)
    assert torch.equal(P.pyramid_frames(xd, bgd, bgi, **kw), got)                                # and two runs give the same bytes
    host = got.cpu().numpy()
    assert host.shape == (4, 128, 64, 3) and host.dtype.name == "uint8"
    assert int((got == 0).sum()) > 0 and int((got == 255).sum()) > 0                             # (the sums leave [0, 1]: both ends saturate)
    kw["antialias"] = True
    same(P.pyramid_frames(xd, bgd, bgi, rounding="nearest", as_float=True, **kw),
         pyramid_frames_restated(x, bg, bgi, rounding="nearest", as_float_=True, **kw), "antialias, nearest, as_float")


def test_render_views_shaped_input(pkg):
    x, bg = values((2, 3), 2, 4, 8, 8, 8)
    bgi = torch.tensor([[1, 0, 1], [0, 0, 1]])
    kw = dict(blur=(5, nine_sigmas(6, 8)), bg_pad=(2, 2, 3, 3))
    for nhwc in (0, 1):
        got = pkg.pyramid_frames(to_dev(layout(x, nhwc)), to_dev(bg), bgi, **kw)
        assert got.shape == (2, 3, 8, 8, 3)
        same(got, pyramid_frames_restated(x, bg, bgi, **kw), nhwc)
    fgi = torch.tensor([[5, 0], [3, 3]])                                                         # flat over (B,N)
    kw["blur"] = (5, nine_sigmas(4, 9))
    got = P.pyramid_frames(to_dev(layout(x, 1)), to_dev(bg), bgi[:, :2], fg_index=fgi, as_float=True, **kw)
    assert got.shape == (2, 2, 3, 8, 8)
    same(got, pyramid_frames_restated(x, bg, bgi[:, :2], fg_index=fgi, as_float_=True, **kw), "fg_index")


def test_nan_in_a_mask_gives_zero_bytes_within_the_cascades_reach_only(pkg):
    g = torch.Generator().manual_seed(11)
    x = torch.rand((2, 4, 37, 41), generator=g)
    bg = torch.rand((2, 3, 37, 41), generator=g)
    kw = dict(blur=(7, nine_sigmas(2, 11)), bg_pad=4)
    clean = P.pyramid_frames(to_dev(x), to_dev(bg), [1, 0], **kw).cpu()
    x[0, 3, 18, 20] = float("nan")
    got = P.pyramid_frames(to_dev(x), to_dev(bg), [1, 0], **kw)
    same(got, pyramid_frames_restated(x, bg, [1, 0], **kw), "NaN")
    got = got.cpu()
    reach = torch.zeros((2, 37, 41), dtype=torch.bool)
    reach[0, 18 - 9:18 + 10, 20 - 9:20 + 10] = True                                              # three levels of radius 3 (a tap of 0 times NaN is NaN)
    assert bool((got[reach] == 0).all()) and torch.equal(got[~reach], clean[~reach])
    assert int((clean[reach] != 0).sum()) > 0


def test_identity_levels_are_the_plain_blend(pkg):
    g = torch.Generator().manual_seed(12)
    x, bg = torch.rand((3, 4, 16, 12), generator=g), torch.rand((2, 3, 16, 12), generator=g)
    want = quantize(bg[[0, 1, 1]] * (1 - x[:, 3:]) + x[:, :3] * x[:, 3:]).permute(0, 2, 3, 1).contiguous()
    same(P.pyramid_frames(to_dev(x), to_dev(bg), [0, 1, 1], blur=torch.ones(1), bg_pad=0), want, "one-tap kernels, no pad")
