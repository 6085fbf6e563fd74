"""Greyscale, 4:4:4 and 4:2:2 JPEG files and the round trip of the two colour ones on the MI355X (csrc/mm_jpeg.hip with the MCU as a
template parameter) against the numpy restatement (tests/test_jpeg_modes_host.py) and, where Pillow imports, against Pillow: whole files
with ==, whole tensors with torch.equal, no tolerance -- nothing on either side is rounded in floating point.

Shapes are the host file's.  Each runs with the six contents as one batch, whose streams have different lengths.  5 x 7 masks of 35 bytes
start at every byte alignment; 257 masks of 8 x 8, one mask of 136 x 128 (272 blocks) and one 256 x 256 noise mask at quality 100 (a stream
of several hundred chunks, larger than LDS) are where the frame, block and chunk scans start another pass in a layout of one block an MCU."""
import functools
import importlib
import io

import numpy as np
import pytest
import torch

from test_gpu_export import to_dev
from test_gpu_jpeg_roundtrip import render_like
from test_jpeg_host import differ
from test_jpeg_modes_host import DECODE_422_SHAPES, LAYOUTS, SHAPES, contents_of, files_restated, frame_of, roundtrip_restated

pytestmark = pytest.mark.gpu

J = importlib.import_module("3d-magic-mirror_amd.jpeg")

try:
    from PIL import Image
except ImportError:                                              # the restatement is then the only yardstick (it is held to Pillow where Pillow is)
    Image = None


def keywords(layout):
    return dict(mode="L") if layout == "L" else dict(subsampling=layout)


@functools.lru_cache(maxsize=None)
def batch_of(H, W, layout):
    """the six contents at one shape, (6,H,W) or (6,H,W,3) uint8; made once and left unchanged"""
    return torch.from_numpy(np.stack([frame_of(kind, H, W, layout) for kind in contents_of(layout)]))


@functools.lru_cache(maxsize=None)
def restated(H, W, quality, layout):
    return tuple(files_restated(batch_of(H, W, layout), quality, **keywords(layout)))


@functools.lru_cache(maxsize=None)
def reopened(H, W, quality, layout):
    return torch.from_numpy(roundtrip_restated(batch_of(H, W, layout), quality, layout))


def pillow_file(f, quality, layout):
    buf = io.BytesIO()
    Image.fromarray(f).save(buf, "JPEG", quality=quality, **({} if layout == "L" else dict(subsampling=layout)))
    return buf.getvalue()


def held(batch, frames, quality, layout, want=None):
    """the device's files are the restatement's and, where Pillow imports, Pillow's"""
    want = files_restated(frames, quality, **keywords(layout)) if want is None else want
    tail = frames.shape[-2:] if layout == "L" else frames.shape[-3:]
    f = frames.cpu().numpy().reshape((-1,) + tuple(tail))
    assert isinstance(batch, J.JpegBatch) and len(batch) == len(want) == f.shape[0]
    assert batch.offsets[0] == 0 and batch.offsets[-1] == sum(len(w) for w in want) == batch.buffer.numel()
    for i, w in enumerate(want):
        got = batch[i]
        assert got == w, (i, quality, layout, differ(got, w))
        if Image is not None:
            theirs = pillow_file(f[i], quality, layout)
            assert got == theirs, (i, quality, layout, "Pillow", differ(got, theirs))


def decoded_held(got, frames, quality, layout, want=None):
    """the device's frames are the restatement's and, where Pillow imports, Pillow's reopened files"""
    want = torch.from_numpy(roundtrip_restated(frames, quality, layout)) if want is None else want
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == frames.shape
    g = got.cpu()
    assert torch.equal(g, want), (quality, layout, int((g != want).sum()))
    if Image is not None:
        f, gn = frames.cpu().numpy().reshape((-1,) + tuple(frames.shape[-3:])), g.numpy().reshape((-1,) + tuple(frames.shape[-3:]))
        for i in range(f.shape[0]):
            with Image.open(io.BytesIO(pillow_file(f[i], quality, layout))) as im:
                assert np.array_equal(gn[i], np.asarray(im.convert("RGB"))), (i, quality, layout, "Pillow")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_and_contents(pkg, H, W, layout):
    x = to_dev(batch_of(H, W, layout))
    for q in (100, 30):
        batch = pkg.encode_jpeg(x, q, **keywords(layout))
        assert batch.shape == (6,)
        held(batch, batch_of(H, W, layout), q, layout, restated(H, W, q, layout))
    assert torch.equal(x.cpu(), batch_of(H, W, layout))          # the frames are left alone


def test_masks_at_every_byte_alignment(pkg):
    g = torch.Generator().manual_seed(5)
    m = torch.randint(0, 256, (5, 5, 7), generator=g, dtype=torch.uint8)
    m[3] = 255                                                   # a short file among longer ones
    store = torch.zeros((5 * 35 + 1,), dtype=torch.uint8)
    store[1:] = m.reshape(-1)
    d = to_dev(store)[1:].view(5, 5, 7)                          # mask i starts at byte 1 + 35 i of an aligned allocation
    assert d.is_contiguous() and len({(d.data_ptr() + 35 * i) % 4 for i in range(5)}) == 4
    held(pkg.encode_jpeg(d, 90, mode="L"), m, 90, "L")
    assert torch.equal(d.cpu(), m)


def test_many_small_masks(pkg):
    """257 frames: the scan of the files' lengths starts a second pass"""
    m = torch.randint(0, 256, (257, 8, 8), generator=torch.Generator().manual_seed(257), dtype=torch.uint8)
    held(pkg.encode_jpeg(to_dev(m), mode="L"), m, 100, "L")


def test_one_mask_of_272_blocks(pkg):
    """136 x 128 is 17 x 16 blocks: the scan of a frame's bit counts starts a second pass, and the code kernels a second workgroup"""
    assert J.lower_jpeg(136, 128, 100, "L")["blocks"] == 272
    m = torch.from_numpy(np.stack([frame_of(kind, 136, 128, "L") for kind in ("noise", "blob")]))
    for q in (100, 30):
        held(pkg.encode_jpeg(to_dev(m), q, mode="L"), m, q, "L")


def test_one_large_noise_mask(pkg):
    """256 x 256 noise at quality 100: 1024 blocks in 208 chunks, a hundred of which hold bytes -- a stream of 100 KB, more than the 64 KB
    of LDS a workgroup can declare: it lives in the workspace"""
    m = torch.randint(0, 256, (1, 256, 256), generator=torch.Generator().manual_seed(256), dtype=torch.uint8)
    want = files_restated(m, 100, mode="L")
    low = J.lower_jpeg(256, 256, 100, "L")
    assert low["chunks"] == 208 and len(want[0]) - len(low["header"]) > 64 * 1024
    held(pkg.encode_jpeg(to_dev(m), 100, mode="L"), m, 100, "L", want)


@pytest.mark.parametrize("layout,shapes", (("4:4:4", SHAPES), ("4:2:2", DECODE_422_SHAPES)))
def test_roundtrip_shapes_and_contents(pkg, layout, shapes):
    for H, W in shapes:
        frames = batch_of(H, W, layout)
        x = to_dev(frames)
        for q in (100, 30):
            decoded_held(pkg.jpeg_roundtrip(x, q, subsampling=layout), frames, q, layout, reopened(H, W, q, layout))
        got = pkg.jpeg_roundtrip(x, 30, as_float=True, subsampling=layout)
        assert got.dtype == torch.float32 and got.shape == (6, 3, H, W)
        assert torch.equal(got.cpu(), reopened(H, W, 30, layout).movedim(-1, -3).float() / 255)      # v / 255 in planes
        assert torch.equal(x.cpu(), frames)


@pytest.mark.parametrize("layout", ("4:4:4", "4:2:2"))
@pytest.mark.parametrize("H,W,q", ((17, 23, 75), (3, 4, 100), (128, 64, 100)))
def test_files_from_the_same_pass(pkg, H, W, q, layout):
    frames = batch_of(H, W, layout)
    x = to_dev(frames)
    decoded, batch = pkg.jpeg_roundtrip(x, q, files=True, subsampling=layout)
    want = pkg.encode_jpeg(x, q, subsampling=layout)
    assert isinstance(batch, J.JpegBatch) and batch.offsets == want.offsets and torch.equal(batch.buffer, want.buffer) and batch.shape == want.shape
    held(batch, frames, q, layout)
    assert torch.equal(decoded, pkg.jpeg_roundtrip(x, q, subsampling=layout))
    decoded_held(decoded, frames, q, layout)
    as_planes, again = pkg.jpeg_roundtrip(x, q, as_float=True, files=True, subsampling=layout)
    assert torch.equal(as_planes.cpu(), decoded.cpu().movedim(-1, -3).float() / 255) and list(again) == list(want)


def test_defaults_and_pillows_ints(pkg):
    frames = batch_of(17, 23, "4:4:4")
    x = to_dev(frames)
    plain = pkg.encode_jpeg(x)
    for kw in (dict(mode="RGB", subsampling="4:2:0"), dict(subsampling=2), dict(quality=100, mode="RGB")):
        other = pkg.encode_jpeg(x, **kw)
        assert other.offsets == plain.offsets and torch.equal(other.buffer, plain.buffer), kw
    assert list(plain) == files_restated(frames, 100)
    for k, s in enumerate(J.SUBSAMPLINGS):
        assert list(pkg.encode_jpeg(x, 75, subsampling=k)) == list(pkg.encode_jpeg(x, 75, subsampling=s))
        assert torch.equal(pkg.jpeg_roundtrip(x, 75, subsampling=k), pkg.jpeg_roundtrip(x, 75, subsampling=s))
    assert torch.equal(pkg.jpeg_roundtrip(x), pkg.jpeg_roundtrip(x, 100, "RGB", False, False, "4:2:0"))
    assert len({tuple(pkg.encode_jpeg(x, 75, subsampling=s)) for s in J.SUBSAMPLINGS}) == 3          # three different sets of files


@pytest.mark.parametrize("layout", LAYOUTS + ("4:2:0",))
def test_two_calls_are_bitwise_identical(pkg, layout):
    x = to_dev(batch_of(24, 40, "L" if layout == "L" else "4:4:4"))
    first, second = (pkg.encode_jpeg(x, 90, **keywords(layout)) for _ in range(2))
    assert first.offsets == second.offsets and torch.equal(first.buffer, second.buffer)
    if layout != "L":
        assert torch.equal(pkg.jpeg_roundtrip(x, 90, subsampling=layout), pkg.jpeg_roundtrip(x, 90, subsampling=layout))


def test_leading_dimensions_and_other_strides(pkg):
    x = torch.randint(0, 256, (2, 3, 17, 23, 3), generator=torch.Generator().manual_seed(23), dtype=torch.uint8)
    m = x[..., 0].contiguous()
    batch = pkg.encode_jpeg(to_dev(m), 75, mode="L")
    assert batch.shape == (2, 3) and len(batch) == 6
    held(batch, m, 75, "L")
    held(pkg.encode_jpeg(to_dev(x)[..., 0], 75, mode="L"), m, 75, "L")                               # a channel of the frames as a mask: strided
    batch = pkg.encode_jpeg(to_dev(x), 75, subsampling="4:2:2")
    assert batch.shape == (2, 3)
    held(batch, x, 75, "4:2:2")
    got = pkg.jpeg_roundtrip(to_dev(x), 75, subsampling="4:2:2")
    assert got.shape == (2, 3, 17, 23, 3) and pkg.jpeg_roundtrip(to_dev(x), 75, as_float=True, subsampling="4:4:4").shape == (2, 3, 3, 17, 23)
    decoded_held(got, x, 75, "4:2:2")


@pytest.mark.parametrize("white", (False, True))
def test_recon_scores_as_saved_with_files(pkg, white):
    pred, gt = (to_dev(t) for t in render_like(4, 17, 23))
    s, iou, saved = pkg.recon_scores_as_saved(pred, gt, white_gt=white, files=True)
    s0, iou0 = pkg.recon_scores_as_saved(pred, gt, white_gt=white)
    assert torch.equal(s, s0) and torch.equal(iou, iou0) and s.shape == (4,)
    assert len(saved) == 4 and all(isinstance(b, J.JpegBatch) and len(b) == 4 for b in saved)
    ori, ori_mask = pkg.export_images(gt, "rgb+mask", rounding="trunc", white=white)
    rec, rec_mask = pkg.export_images(pred, "rgb+mask", rounding="trunc")
    for batch, frames, layout in zip(saved, (ori, ori_mask, rec, rec_mask), ("4:2:0", "L", "4:2:0", "L")):
        f = frames.cpu()
        assert list(batch) == files_restated(f, 100, **keywords(layout))
        if Image is not None:                                    # Pillow's files of the exported bytes
            assert list(batch) == [pillow_file(one, 100, layout) for one in f.numpy()]
