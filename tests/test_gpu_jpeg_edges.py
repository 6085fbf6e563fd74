"""The JPEG encoder on the MI355X (csrc/mm_jpeg.hip) on the constructed inputs of tests/test_jpeg_edges_host.py, which reach each discrete
path of the parallel entropy coder by construction, and at the sizes where a scan starts another pass: the device's files equal the
restatement's and Pillow's byte for byte (``test_gpu_jpeg.held``), no tolerance.

The cases of one (H, W, quality) go through ``encode_jpeg`` as ONE batch, so streams of different shapes lie side by side in a call.
Beyond the cases: 256, 257 and 513 frames (``jpeg_file_offsets_kernel`` scans the lengths 256 at a time with a carry); frames of 258 and
768 blocks (``jpeg_bit_offsets_kernel``: one block past a pass, and whole passes); one frame whose stream before stuffing is longer than
256 chunks of 1024 bytes with a 0xFF beyond them (``jpeg_place_kernel``'s carry under a chunk that holds bytes); and the streams of
exactly 1024, 1025 and 2048 bytes as the first and the last frame of a batch (they are a batch's only frame among the cases), where
EOI abuts the next file's header."""
import functools

import numpy as np
import pytest
import torch

import test_jpeg_edges_host as E
from test_gpu_export import to_dev
from test_gpu_jpeg import held
from test_jpeg_host import jpeg_restated

pytestmark = pytest.mark.gpu


# the cases of equal (H, W, quality), in the table's order (written out so that collecting this file builds nothing)
GROUPS = (("dc_extremes",), ("ac_extremes", "ties"), ("long_runs_q75",), ("long_runs_q50",), ("writer_shapes",), ("ends_mod4",), ("ends_1024",),
          ("ends_1025",), ("ends_2048",), ("last_ff_padded", "many_frames"), ("ff_placement",), ("colour_rounding",))


def test_groups_are_the_cases_by_shape_and_quality():
    out = {}
    for name in E.CASES:
        frames, quality = E.case(name)[:2]
        out.setdefault(frames.shape[1:3] + (quality,), []).append(name)
    assert tuple(tuple(v) for v in out.values()) == GROUPS


def same_files(a, b):
    return a.offsets == b.offsets and torch.equal(a.buffer, b.buffer)


@pytest.mark.parametrize("names", GROUPS, ids="+".join)
def test_cases_as_one_batch(pkg, names):
    x = torch.from_numpy(np.concatenate([E.case(name)[0] for name in names]))
    want = [f for name in names for f in E.case(name)[2]]
    quality = E.case(names[0])[1]
    d = to_dev(x)
    batch = pkg.encode_jpeg(d, quality)
    held(batch, x, quality, want)
    assert same_files(pkg.encode_jpeg(d, quality), batch), names # two runs give the same bytes
    assert torch.equal(d.cpu(), x)


@functools.lru_cache(maxsize=None)
def tiny_frames():
    """(513,8,8,3) noise, and its files at quality 100: made once, shared by the three counts"""
    x = torch.randint(0, 256, (513, 8, 8, 3), generator=torch.Generator().manual_seed(513), dtype=torch.uint8)
    return x, tuple(jpeg_restated(x, 100))


@pytest.mark.parametrize("n", (256, 257, 513))
def test_frame_counts_around_the_offset_scan(pkg, n):
    x, want = tiny_frames()[0][:n], list(tiny_frames()[1][:n])
    assert len({len(w) for w in want}) > 1                       # files of different lengths: the offsets are no multiples of one
    batch = pkg.encode_jpeg(to_dev(x), 100)
    assert batch.offsets == [0] + np.cumsum([len(w) for w in want]).tolist()
    held(batch, x, 100, want)


@pytest.mark.parametrize("W,blocks", ((688, 258), (2048, 768)))
def test_block_counts_around_the_bit_offset_scan(pkg, W, blocks):
    assert E.J.lower_jpeg(16, W, 100)["blocks"] == blocks
    x = torch.randint(0, 256, (1, 16, W, 3), generator=torch.Generator().manual_seed(W), dtype=torch.uint8)
    held(pkg.encode_jpeg(to_dev(x), 100), x, 100)


def test_stream_of_more_than_256_chunks(pkg):
    # 336 x 400, 525 MCUs: of the noise frames (seed H W) of whole MCUs, by MCU count and then squareness, the first that meets both conditions;
    # 256 x 256 has half the bytes, 288 x 464 is long enough and has no 0xFF beyond the 256th chunk
    H, W = 336, 400
    x = torch.randint(0, 256, (1, H, W, 3), generator=torch.Generator().manual_seed(H * W), dtype=torch.uint8)
    c = {}
    want = jpeg_restated(x, 100, c)
    s = c["streams"][0]
    assert s["raw_bytes"] > 256 * 1024 and s["ff_at"][-1] >= 256 * 1024
    assert E.J.lower_jpeg(H, W, 100)["chunks"] > 512             # the chunk scan runs a third pass, over empty chunks
    held(pkg.encode_jpeg(to_dev(x), 100), x, 100, want)


@pytest.mark.parametrize("name", ("ends_1024", "ends_1025", "ends_2048"))
def test_stream_ends_as_first_and_last_frame(pkg, name):
    tuned, _, file, _, _ = E.case(name)
    W = tuned.shape[2]
    x = torch.from_numpy(np.stack([tuned[0], E.noise_then_grey(1, W), E.noise_then_grey(3, W), tuned[0]]))
    want = jpeg_restated(x, 100)
    assert want[0] == want[3] == file[0] and len({len(w) for w in want}) > 1
    held(pkg.encode_jpeg(to_dev(x), 100), x, 100, want)
