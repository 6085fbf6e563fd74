"""The JPEG round trip on the MI355X (``jpeg_roundtrip`` over csrc/mm_jpeg.hip) against the numpy restatement of libjpeg's decoder
(tests/test_jpeg_roundtrip_host.py) and, where Pillow imports, against Pillow's reopened file: whole tensors, torch.equal, no tolerance --
nothing on either side is rounded in floating point.

Shapes are the host file's, the smallest at which each decode rule can go wrong: W <= 4 takes plain replication, 40 x 5 is the smallest
"fancy" case, 3 x 40 and 1 x 40 have two chroma rows and one, 31 x 18, 18 x 31 and 16 x 33 put chroma neighbours across an MCU boundary and
leave a last real chroma row above padding.  Each shape runs with every content as one batch.  5 x 7 frames start at every byte alignment
(and their 105-byte outputs put every frame's first dword across a frame boundary); 50 frames of 16 x 16 and 257 frames of 8 x 8 span the
grids; one 256 x 256 noise frame has many workgroups per frame."""
import functools
import importlib

import numpy as np
import pytest
import torch

from test_gpu_export import to_dev
from test_jpeg_host import CONTENTS, content
from test_jpeg_roundtrip_host import COLOUR_SHAPES, GREY_CONTENTS, GREY_SHAPES, grey_content, pillow_roundtrip, roundtrip_restated

pytestmark = pytest.mark.gpu

J = importlib.import_module("3d-magic-mirror_amd.jpeg")
S = importlib.import_module("3d-magic-mirror_amd.synthetic")

try:
    from PIL import Image
except ImportError:                                              # the restatement is then the only yardstick (it is held to Pillow where Pillow is)
    Image = None


@functools.lru_cache(maxsize=None)
def batch_of(H, W, mode="RGB"):
    """every content at one shape, (6,H,W,3) or (4,H,W) uint8; made once and left unchanged"""
    if mode == "RGB":
        return torch.from_numpy(np.stack([content(kind, H, W) for kind in CONTENTS]))
    return torch.from_numpy(np.stack([grey_content(kind, H, W) for kind in GREY_CONTENTS]))


@functools.lru_cache(maxsize=None)
def restated(H, W, quality, mode="RGB"):
    return torch.from_numpy(roundtrip_restated(batch_of(H, W, mode), quality, mode))


def held(got, frames, quality, mode="RGB", want=None):
    """the device's frames are the restatement's and, where Pillow imports, Pillow's reopened files"""
    want = torch.from_numpy(roundtrip_restated(frames, quality, mode)) if want is None else want
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == frames.shape
    g = got.cpu()
    assert torch.equal(g, want), (quality, mode, int((g != want).sum()))
    if Image is not None:
        tail = frames.shape[-3:] if mode == "RGB" else frames.shape[-2:]
        f, gn = frames.cpu().numpy().reshape((-1,) + tuple(tail)), g.numpy().reshape((-1,) + tuple(tail))
        for i in range(f.shape[0]):
            assert np.array_equal(gn[i], pillow_roundtrip(f[i], quality)), (i, quality, mode, "Pillow")


def planes(u8, mode="RGB"):
    """to_tensor of the reopened images: float32 v / 255, (...,3,H,W) or (...,H,W)"""
    return (u8.movedim(-1, -3) if mode == "RGB" else u8).float() / 255


@pytest.mark.parametrize("H,W", COLOUR_SHAPES)
def test_colour_shapes_and_contents(pkg, H, W):
    x = to_dev(batch_of(H, W))
    for q in (100, 30) + ((95, 1) if (H, W) == (17, 23) else ()):
        held(pkg.jpeg_roundtrip(x, q), batch_of(H, W), q, "RGB", restated(H, W, q))
    got = pkg.jpeg_roundtrip(x, 30, as_float=True)
    assert got.dtype == torch.float32 and got.shape == (6, 3, H, W) and torch.equal(got.cpu(), planes(restated(H, W, 30)))
    assert torch.equal(x.cpu(), batch_of(H, W))                  # the frames are left alone


@pytest.mark.parametrize("H,W", GREY_SHAPES)
def test_grey_shapes_and_contents(pkg, H, W):
    x = to_dev(batch_of(H, W, "L"))
    for q in (100, 30) + ((95, 1) if (H, W) == (17, 23) else ()):
        held(pkg.jpeg_roundtrip(x, q, mode="L"), batch_of(H, W, "L"), q, "L", restated(H, W, q, "L"))
    got = pkg.jpeg_roundtrip(x, 30, mode="L", as_float=True)
    assert got.dtype == torch.float32 and got.shape == (4, H, W) and torch.equal(got.cpu(), planes(restated(H, W, 30, "L"), "L"))
    assert torch.equal(x.cpu(), batch_of(H, W, "L"))


@pytest.mark.parametrize("H,W,q", ((17, 23, 75), (40, 3, 100), (128, 64, 100)))
def test_files_from_the_same_pass(pkg, H, W, q):
    x = to_dev(batch_of(H, W))
    decoded, batch = pkg.jpeg_roundtrip(x, q, files=True)
    want = pkg.encode_jpeg(x, q)
    assert isinstance(batch, J.JpegBatch) and batch.offsets == want.offsets and torch.equal(batch.buffer, want.buffer) and batch.shape == want.shape
    assert torch.equal(decoded, pkg.jpeg_roundtrip(x, q))        # the frames the files' own coefficients decode to
    held(decoded, batch_of(H, W), q)
    as_planes, again = pkg.jpeg_roundtrip(x, q, as_float=True, files=True)
    assert torch.equal(as_planes.cpu(), planes(decoded.cpu())) and list(again) == list(want)
    if Image is not None:                                        # and Pillow opens those files to those frames
        import io
        for i in range(len(batch)):
            with Image.open(io.BytesIO(batch[i])) as im:
                assert np.array_equal(np.asarray(im.convert("RGB")), decoded[i].cpu().numpy())


def test_frames_at_every_byte_alignment(pkg):
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (5, 5, 7, 3), generator=g, dtype=torch.uint8)
    store = torch.zeros((5 * 105 + 1,), dtype=torch.uint8)
    store[1:] = x.reshape(-1)
    d = to_dev(store)[1:].view(5, 5, 7, 3)                       # frame i starts at byte 1 + 105 i of an aligned allocation
    assert d.is_contiguous() and len({(d.data_ptr() + 105 * i) % 4 for i in range(5)}) == 4
    held(pkg.jpeg_roundtrip(d, 90), x, 90)
    m = x[..., 0].contiguous()                                   # masks of 35 bytes, likewise
    store = torch.zeros((5 * 35 + 1,), dtype=torch.uint8)
    store[1:] = m.reshape(-1)
    dm = to_dev(store)[1:].view(5, 5, 7)
    assert len({(dm.data_ptr() + 35 * i) % 4 for i in range(5)}) == 4
    held(pkg.jpeg_roundtrip(dm, 90, mode="L"), m, 90, "L")


@pytest.mark.parametrize("n,side", ((50, 16), (257, 8)))
def test_many_small_frames(pkg, n, side):
    g = torch.Generator().manual_seed(n)
    x = torch.randint(0, 256, (n, side, side, 3), generator=g, dtype=torch.uint8)
    held(pkg.jpeg_roundtrip(to_dev(x)), x, 100)
    held(pkg.jpeg_roundtrip(to_dev(x[..., 1].contiguous()), mode="L"), x[..., 1].contiguous(), 100, "L")


def test_one_large_frame_twice(pkg):
    x = torch.randint(0, 256, (1, 256, 256, 3), generator=torch.Generator().manual_seed(256), dtype=torch.uint8)
    d = to_dev(x)
    first = pkg.jpeg_roundtrip(d, 100)
    held(first, x, 100)
    assert torch.equal(pkg.jpeg_roundtrip(d, 100), first)        # two calls give the same bytes
    m = to_dev(x[..., 2].contiguous())
    first = pkg.jpeg_roundtrip(m, 100, mode="L")
    held(first, x[..., 2].contiguous(), 100, "L")
    assert torch.equal(pkg.jpeg_roundtrip(m, 100, mode="L"), first) and torch.equal(m.cpu(), x[..., 2])


def test_leading_dimensions_and_other_strides(pkg):
    g = torch.Generator().manual_seed(23)
    x = torch.randint(0, 256, (2, 3, 17, 23, 3), generator=g, dtype=torch.uint8)
    got = pkg.jpeg_roundtrip(to_dev(x), 75)
    assert got.shape == (2, 3, 17, 23, 3)
    held(got, x, 75)
    assert pkg.jpeg_roundtrip(to_dev(x), 75, as_float=True).shape == (2, 3, 3, 17, 23)
    decoded, batch = pkg.jpeg_roundtrip(to_dev(x), 75, files=True)
    assert batch.shape == (2, 3) and torch.equal(decoded, got)
    m = x[..., 0].contiguous()
    got = pkg.jpeg_roundtrip(to_dev(m), 75, mode="L")
    assert got.shape == (2, 3, 17, 23) and pkg.jpeg_roundtrip(to_dev(m), 75, mode="L", as_float=True).shape == (2, 3, 17, 23)
    held(got, m, 75, "L")
    view = to_dev(x.permute(0, 1, 4, 2, 3).contiguous()).permute(0, 1, 3, 4, 2)        # not contiguous
    assert not view.is_contiguous()
    held(pkg.jpeg_roundtrip(view, 75), x, 75)
    held(pkg.jpeg_roundtrip(to_dev(x)[..., 0], 75, mode="L"), m, 75, "L")              # a channel of the frames as a mask: strided


def render_like(B, H, W):
    """(B,4,H,W) pred and gt: synthetic's ground truth, and the same dimmed a little with its mask moved by a pixel"""
    gt = S.synthetic_batch(torch.zeros(4, 3), B, H, W, seed=11)[1].float().contiguous()
    pred = torch.cat([(0.9 * gt[:, :3] + 0.05).clamp(0, 1), torch.roll(gt[:, 3:], (1, 1), (2, 3))], 1)
    return pred, gt


@pytest.mark.parametrize("white", (False, True))
def test_recon_scores_as_saved_is_the_composition(pkg, white):
    pred, gt = (to_dev(t) for t in render_like(3, 128, 64))
    s, iou = pkg.recon_scores_as_saved(pred, gt, white_gt=white)
    assert s.shape == (3,) and iou.shape == (3,) and s.is_cuda
    ori, ori_mask = pkg.export_images(gt, "rgb+mask", rounding="trunc", white=white)
    rec, rec_mask = pkg.export_images(pred, "rgb+mask", rounding="trunc")
    ori, rec = pkg.jpeg_roundtrip(ori, 100, "RGB", as_float=True), pkg.jpeg_roundtrip(rec, 100, "RGB", as_float=True)
    ori_mask, rec_mask = pkg.jpeg_roundtrip(ori_mask, 100, "L", as_float=True), pkg.jpeg_roundtrip(rec_mask, 100, "L", as_float=True)
    assert torch.equal(s, pkg.ssim(ori, rec, data_range=1, size_average=False))
    # the mask-IoU kernel recon_scores uses, through recon_scores: channel 3 of (pred, gt) is (rhs, lhs)
    assert torch.equal(iou, pkg.recon_scores(torch.cat([rec, rec_mask[:, None]], 1), torch.cat([ori, ori_mask[:, None]], 1))[1])
    sums = torch.stack([(ori_mask * rec_mask).flatten(1).sum(1), (ori_mask + rec_mask - ori_mask * rec_mask).flatten(1).sum(1)])
    assert torch.allclose(iou, sums[0] / (sums[1] + 1e-10), rtol=1e-5, atol=0)
    s75, iou75 = pkg.recon_scores_as_saved(pred, gt, quality=75, white_gt=white)
    assert not torch.equal(s75, s) and torch.isfinite(s75).all() and torch.isfinite(iou75).all()      # another quality, other numbers


def test_recon_scores_as_saved_differs_from_recon_scores(pkg):
    """the point of the feature: the numbers of the saved files are not the numbers of the tensors"""
    pred, gt = (to_dev(t) for t in render_like(3, 128, 64))
    s, iou = pkg.recon_scores_as_saved(pred, gt)
    s0, iou0 = pkg.recon_scores(pred, gt)
    assert not torch.equal(s, s0) and not torch.equal(iou, iou0)
    assert torch.isfinite(s).all() and ((0 <= iou) & (iou <= 1)).all()
    again = pkg.recon_scores_as_saved(pred, gt)
    assert torch.equal(again[0], s) and torch.equal(again[1], iou)
    host = pkg.recon_scores_as_saved(pred.cpu(), gt.cpu())       # host tensors: moved to the device, results back on the host
    assert not host[0].is_cuda and torch.equal(host[0], s.cpu()) and torch.equal(host[1], iou.cpu())
