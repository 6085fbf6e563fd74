"""The JPEG encoder on the MI355X (csrc/mm_jpeg.hip) against the numpy restatement (tests/test_jpeg_host.py): the device's files equal the
restatement's byte for byte, whole files, unconditionally -- nothing on either side is rounded in floating point, so there is no tolerance --
and, where Pillow imports, Pillow's too.

Shapes are test_jpeg_host's, the smallest that reach each path: 1 x 1 is one MCU with three dummy luma blocks; 17 x 23 has dummies on both
edges; 24 x 40 and 40 x 24 have an even H with H mod 16 = 8, where chroma rows replicate the downsampled row; 33 x 9 and 50 x 70 have odd
numbers of MCUs; 128 x 64 is the call site.  Each shape runs with every content of that file as one batch of six frames, whose streams have
different lengths.  5 x 7 frames of 105 bytes start at every byte alignment; 50 frames of 16 x 16 span the per-frame kernels' grids; one
256 x 256 noise frame at quality 100 has a stream larger than LDS, several workgroups of blocks per scan and some hundred chunks.

These inputs reach the entropy coder's discrete paths by chance.  tests/test_gpu_jpeg_edges.py runs the constructed cases of
tests/test_jpeg_edges_host.py, one per path, and the sizes at which each scan starts another pass (257 frames, 258 blocks, 257 chunks that hold bytes)."""
import functools
import importlib
import io

import numpy as np
import pytest
import torch

from test_gpu_export import to_dev
from test_jpeg_host import CONTENTS, SHAPES, content, differ, jpeg_restated

pytestmark = pytest.mark.gpu

J = importlib.import_module("3d-magic-mirror_amd.jpeg")

try:
    from PIL import Image
except ImportError:                                              # the restatement is then the only yardstick (it is held to Pillow where Pillow is)
    Image = None


@functools.lru_cache(maxsize=None)
def batch_of(H, W):
    """the six contents at one shape, (6,H,W,3) uint8; made once and left unchanged"""
    x = torch.from_numpy(np.stack([content(kind, H, W) for kind in CONTENTS]))
    return x


@functools.lru_cache(maxsize=None)
def restated(H, W, quality):
    return tuple(jpeg_restated(batch_of(H, W), quality))


def held(batch, frames, quality, want=None):
    """the device's files are the restatement's and, where Pillow imports, Pillow's"""
    want = jpeg_restated(frames, quality) if want is None else want
    f = frames.cpu().numpy().reshape((-1,) + tuple(frames.shape[-3:]))
    assert len(batch) == len(want) == f.shape[0]
    assert batch.offsets[0] == 0 and batch.offsets[-1] == sum(len(w) for w in want) == batch.buffer.numel()
    for i, w in enumerate(want):
        got = batch[i]
        assert got == w, (i, quality, differ(got, w))
        if Image is not None:
            buf = io.BytesIO()
            Image.fromarray(f[i]).save(buf, "JPEG", quality=quality)
            assert got == buf.getvalue(), (i, quality, "Pillow", differ(got, buf.getvalue()))


@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_and_contents(pkg, H, W):
    x = to_dev(batch_of(H, W))
    for q in (100, 30) + ((95, 1) if (H, W) == (17, 23) else ()):               # quality 1: divisors up to 8 * 255
        held(pkg.encode_jpeg(x, q), batch_of(H, W), q, restated(H, W, q))
    assert torch.equal(x.cpu(), batch_of(H, W))                  # the frames are left alone


def test_frames_at_every_byte_alignment(pkg):
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (5, 5, 7, 3), generator=g, dtype=torch.uint8)
    x[3] = 255                                                   # a short file among longer ones
    store = torch.zeros((5 * 105 + 1,), dtype=torch.uint8)
    store[1:] = x.reshape(-1)
    d = to_dev(store)[1:].view(5, 5, 7, 3)                       # frame i starts at byte 1 + 105 i of an aligned allocation
    assert d.is_contiguous() and len({(d.data_ptr() + 105 * i) % 4 for i in range(5)}) == 4
    batch = pkg.encode_jpeg(d, 90)
    held(batch, x, 90)
    assert len({batch.offsets[i + 1] - batch.offsets[i] for i in range(5)}) > 1


@pytest.mark.parametrize("n", (1, 50))
def test_one_frame_and_fifty(pkg, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randint(0, 256, (n, 16, 16, 3), generator=g, dtype=torch.uint8)
    batch = pkg.encode_jpeg(to_dev(x))
    assert len(batch) == n and batch.shape == (n,)
    held(batch, x, 100)


def test_stream_larger_than_lds(pkg):
    x = torch.randint(0, 256, (1, 256, 256, 3), generator=torch.Generator().manual_seed(256), dtype=torch.uint8)
    c = {}
    want = jpeg_restated(x, 100, c)
    assert len(want[0]) > 64 * 1024 * 2 - 4096 and c["stuffed"] > 100
    d = to_dev(x)
    batch = pkg.encode_jpeg(d, 100)
    held(batch, x, 100, want)
    again = pkg.encode_jpeg(d, 100)                              # two runs give the same bytes
    assert again.offsets == batch.offsets and torch.equal(again.buffer, batch.buffer)


def test_leading_dimensions_and_other_strides(pkg):
    g = torch.Generator().manual_seed(23)
    x = torch.randint(0, 256, (2, 3, 17, 23, 3), generator=g, dtype=torch.uint8)
    batch = pkg.encode_jpeg(to_dev(x), 75)
    assert batch.shape == (2, 3) and len(batch) == 6             # files in row-major order over the leading dimensions
    held(batch, x, 75)
    planes = x.permute(0, 1, 4, 2, 3).contiguous()               # (2,3,3,H,W) memory seen as (2,3,H,W,3): not contiguous
    view = to_dev(planes).permute(0, 1, 3, 4, 2)
    assert not view.is_contiguous() and torch.equal(view.cpu(), x)
    held(pkg.encode_jpeg(view, 75), x, 75)
    wide = to_dev(torch.randint(0, 256, (4, 16, 40, 3), generator=g, dtype=torch.uint8))
    held(pkg.encode_jpeg(wide[:, :, 3:27], 100), wide[:, :, 3:27].cpu().contiguous(), 100)       # a window of wider frames


def test_pyramid_frames_straight_in(pkg):
    P = importlib.import_module("3d-magic-mirror_amd.pyramid")
    g = torch.Generator().manual_seed(7)
    B = 4
    pred, bg = torch.rand((B, 4, 128, 64), generator=g), torch.rand((B, 3, 128, 64), generator=g)
    pred[:, 3] = (pred[:, 3] > 0.5).float()
    frames = pkg.pyramid_frames(to_dev(pred), to_dev(bg), torch.tensor([3, 0, 0, 2]), **P.preset("tool/generate_market_test", B, generator=g))
    assert frames.shape == (B, 128, 64, 3) and frames.dtype == torch.uint8 and frames.is_cuda
    batch = pkg.encode_jpeg(frames)
    held(batch, frames.cpu(), 100)
    if Image is not None:
        for i in range(B):
            with Image.open(io.BytesIO(batch[i])) as im:
                assert im.size == (64, 128) and im.mode == "RGB" and im.format == "JPEG"
