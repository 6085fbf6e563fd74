"""The Poisson blend on the MI355X (csrc/mm_poisson.hip) against the eager torch restatement evaluated on the CPU
(tests/test_poisson_host.py), with torch.equal, bytes and as_float planes alike: every operation is one correctly rounded fp32 multiply,
add or subtract, an exact conversion, or a table value from the host, the file is compiled without contraction, and the cells of one
colour do not read each other, so there is no tolerance to measure.

Shapes are the smallest that reach each path.  1 x 1, 2 x 3 and 3 x 3 are all border (3 x 3 has the one interior cell); 9 x 7 has an odd
width, so the colour that starts a row alternates and every other row of a colour plane ends in a dummy slot; 16 x 12 has an even one;
40 x 33 has 40 x 18 = 720 slots a colour in the first instance (one slot per lane) with lanes left over, and two resize bands and a
remainder.  128 x 64 and 128 x 128 are the call site's shapes with the default sweeps, the instances of 5 and 9 slots per lane, the second
the first plane past 64 KiB of LDS; the largest square the LDS takes runs the instance that keeps x in LDS."""
import importlib

import pytest
import torch

from test_gpu_composite import same, values
from test_gpu_export import layout, to_dev
from test_poisson_host import largest_square, make_mask, poisson_frames_restated

pytestmark = pytest.mark.gpu

P = importlib.import_module("3d-magic-mirror_amd.poisson")
PY = importlib.import_module("3d-magic-mirror_amd.pyramid")
EX = importlib.import_module("3d-magic-mirror_amd.export")

SMALL = {(1, 1): 0, (2, 3): (2, 1, 1, 1), (3, 3): (1, 2, 2, 1), (9, 7): (2, 3, 4, 1), (16, 12): 4, (40, 33): (5, 4, 9, 7)}


def check(x, bg, bgi, nhwc=0, **kw):
    got = P.poisson_frames(to_dev(layout(x, nhwc)), to_dev(bg), bgi, **{k: (to_dev(v) if k == "mask" else v) for k, v in kw.items()})
    kw["as_float_"] = kw.pop("as_float", False)
    same(got, poisson_frames_restated(x, bg, bgi, **kw), (tuple(x.shape), nhwc, {k: v for k, v in kw.items() if k != "mask"}))
    return got


@pytest.mark.parametrize("shape", sorted(SMALL))
def test_small_shapes_eight_sweeps(pkg, shape):
    """NCHW and NHWC renders, 3- and 4-channel backgrounds, repeated indices, both borders, both roundings, as_float, antialias, two
    non-default omegas; the renders hold a NaN and an inf pixel, exact 0s and 1s in the alpha, and k/255 with their fp32 neighbours"""
    H, W = shape
    pad = SMALL[shape]
    fgi, bgi = [2, 0, 2], torch.tensor([1, 1, 0])                                                # repeats, out of order
    for nhwc, bg_C, border, rounding, fl, aa, omega in ((0, 3, "reference", "trunc", False, False, None), (1, 4, "pinned", "nearest", False, True, 1.0),
                                                        (1, 3, "reference", "nearest", True, True, 1.9), (0, 4, "pinned", "trunc", True, False, None)):
        x, bg = values((3,), 2, bg_C, H, W, 7 * H + W + bg_C)
        got = check(x, bg, bgi, nhwc, fg_index=fgi, bg_pad=pad, antialias=aa, border=border, sweeps=8, omega=omega, rounding=rounding, as_float=fl)
        assert got.shape == ((3, 3, H, W) if fl else (3, H, W, 3))


@pytest.mark.parametrize("shape", sorted(SMALL))
def test_masks_given(pkg, shape):
    """mask= as bool and as bytes (any non-zero value is inside), per render: all zero, all one, touching all four edges, speckle"""
    H, W = shape
    x, bg = values((3,), 2, 3, H, W, 11 * H + W)
    for dtype, border, kinds in ((torch.bool, "reference", ("zeros", "ones", "border")), (torch.uint8, "pinned", ("border", "speckle", "zeros")),
                                 (torch.uint8, "reference", ("ones", "ones", "speckle"))):
        m = torch.stack([make_mask(k, H, W, i) for i, k in enumerate(kinds)])
        m = m if dtype == torch.bool else m.to(torch.uint8) * torch.tensor([1, 200, 255], dtype=torch.uint8)[:, None, None]
        check(x, bg, [0, 1, 1], 1, fg_index=[1, 2, 0], mask=m, bg_pad=SMALL[shape], border=border, sweeps=8)


def test_sweeps_zero_and_one(pkg):
    x, bg = values((2,), 2, 3, 9, 7, 3)
    for sweeps in (0, 1):
        for border in ("reference", "pinned"):
            check(x, bg, [1, 0], 1, bg_pad=(2, 3, 4, 1), border=border, sweeps=sweeps)


def test_leading_dimensions(pkg):
    x, bg = values((2, 3), 2, 4, 8, 8, 8)
    bgi = torch.tensor([[1, 0, 1], [0, 0, 1]])
    for nhwc in (0, 1):
        got = check(x, bg, bgi, nhwc, bg_pad=(2, 2, 3, 3), sweeps=8)
        assert got.shape == (2, 3, 8, 8, 3)
    fgi = torch.tensor([[5, 0], [3, 3]])                                                         # flat over (B,N)
    m = torch.stack([make_mask("speckle", 8, 8, i) for i in range(6)]).reshape(2, 3, 8, 8)
    got = check(x, bg, bgi[:, :2], 1, fg_index=fgi, mask=m, bg_pad=1, sweeps=8, border="pinned", as_float=True)
    assert got.shape == (2, 2, 3, 8, 8)
    assert pkg.poisson_frames is P.poisson_frames and pkg.lower_poisson is P.lower_poisson


@pytest.mark.parametrize("shape", ((128, 64), (128, 128)))
def test_call_site_shapes_with_the_default_sweeps(pkg, shape):
    H, W = shape
    x, bg = values((2,), 3, 4, H, W, H + W)
    x[0, :3, H // 2, W // 2] = 0.5                                                               # (frame 0 without its NaN: a whole frame of real bytes)
    x[0, 1, H - 1, 0] = 0.25
    bgi = torch.tensor([2, 0])
    xd, bgd = to_dev(layout(x, 1)), to_dev(bg)
    before = xd.clone(), bgd.clone()
    kw = P.PRESETS["tool/generate_market_test"]
    got = P.poisson_frames(xd, bgd, bgi, **kw)
    same(got, poisson_frames_restated(x, bg, bgi, **kw), "preset")
    assert torch.equal(xd.view(torch.int32), before[0].view(torch.int32)) and torch.equal(bgd, before[1])   # the inputs are left alone
    assert torch.equal(P.poisson_frames(xd, bgd, bgi, **kw), got)                                # and two runs give the same bytes
    assert int((got == 0).sum()) > 0 and int((got == 255).sum()) > 0                             # (the solution leaves [0, 1]: both ends saturate)


def test_largest_plane(pkg):
    n = largest_square()
    x, bg = values((2,), 1, 3, n, n, n)
    x = x[:1]                                                                                    # one frame
    check(x, bg, [0], 1, sweeps=8)
    m = make_mask("border", n, n, 0)[None]
    check(x, bg, [0], 0, mask=m, sweeps=8, border="pinned", rounding="nearest")


def test_nan_in_a_render_pixel(pkg):
    """a NaN in the source reaches b of the pixel and of its four neighbours, and from there every free cell connected to them; the
    quantiser sends them to 0.  The other frame, and the pinned cells, keep their bytes."""
    g = torch.Generator().manual_seed(5)
    x, bg = torch.rand((2, 4, 16, 12), generator=g), torch.rand((2, 3, 16, 12), generator=g)
    m = torch.zeros((2, 16, 12), dtype=torch.bool)
    m[:, 4:12, 3:9] = True
    kw = dict(mask=m, bg_pad=4, border="pinned", sweeps=16)
    clean = check(x, bg, [1, 0], 0, **kw).cpu()
    x[0, 1, 8, 6] = float("nan")
    got = check(x, bg, [1, 0], 0, **kw).cpu()
    assert bool((got[0, 4:12, 3:9, 1] == 0).all()) and int((clean[0, 4:12, 3:9, 1] != 0).sum()) > 0
    got[0, 4:12, 3:9, 1] = clean[0, 4:12, 3:9, 1]
    assert torch.equal(got, clean)


def test_all_zero_mask_pinned_is_the_pyramids_background(pkg):
    """no restatement: every cell pinned, the frames are the quantised level-0 background, which a pyramid of one-tap blurs gives too"""
    g = torch.Generator().manual_seed(4)                                                         # (finite renders: the pyramid multiplies them by the zero mask)
    x, bg = torch.rand((3, 4, 40, 33), generator=g), torch.rand((2, 4, 40, 33), generator=g)
    x[:, 3] = 0
    xd, bgd = to_dev(layout(x, 1)), to_dev(bg)
    for aa, rounding in ((False, "trunc"), (True, "nearest")):
        kw = dict(bg_pad=(5, 4, 9, 7), antialias=aa, rounding=rounding)
        assert torch.equal(P.poisson_frames(xd, bgd, [1, 0, 1], border="pinned", **kw), PY.pyramid_frames(xd, bgd, [1, 0, 1], blur=torch.ones(1), **kw))
    m = torch.zeros((3, 40, 33), dtype=torch.uint8)
    x[:, 3] = 1
    assert torch.equal(P.poisson_frames(to_dev(x), bgd, [1, 0, 1], mask=to_dev(m), border="pinned", bg_pad=(5, 4, 9, 7)),
                       PY.pyramid_frames(xd, bgd, [1, 0, 1], blur=torch.ones(1), bg_pad=(5, 4, 9, 7)))


@pytest.mark.parametrize("shape", ((16, 12), (128, 64)))
def test_all_one_mask_gives_the_render_back(pkg, shape):
    """no restatement: with every cell inside, x = s solves the system (both sides are the same operator with the same zeros outside
    the image), so the default sweeps come back to the render's own bytes within one grey level, whatever the background"""
    H, W = shape
    g = torch.Generator().manual_seed(H)
    x, bg = torch.rand((2, 4, H, W), generator=g), torch.rand((2, 3, H, W), generator=g)
    x[:, 3] = 1
    xd = to_dev(x)
    for border in ("reference", "pinned"):
        got = P.poisson_frames(xd, to_dev(bg), [1, 0], bg_pad=min(16, W - 1), border=border)
        want = EX.export_images(xd, "rgb")
        assert got.shape == want.shape and int((got.int() - want.int()).abs().max()) <= 1
