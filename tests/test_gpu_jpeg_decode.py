"""The JPEG file decoder on the MI355X (``decode_jpeg`` over csrc/mm_jpeg_decode.hip): whole tensors, torch.equal, no tolerance -- nothing on
either side is rounded in floating point.

Yardsticks: the pixels Pillow read back from the fixture's files (tests/golden/jpeg_decode.npz, jpeg_decode_256.npz); the closed loop
``decode_jpeg(encode_jpeg(x)) == jpeg_roundtrip(x)``, which needs no Pillow (both sides are pinned to Pillow by their own tests); and, for
damaged streams only, ``decode_jpeg_host``.  Shapes are the round trip's (the smallest at which each upsampling and edge rule can go wrong),
plus what is the decoder's own: files of different sizes in one call, files starting at every byte alignment inside an ``out=`` that itself
starts at every alignment, 257 files (more than a workgroup of segments, more than one workgroup of blocks), 16 restart intervals in one
file, several Huffman table sets in one call.  The damaged vectors are a handful that the sanitized host program of
tests/test_jpeg_decode_host.py has passed, and they run last."""
import importlib
import io
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_export import DEV, to_dev
from test_gpu_jpeg_roundtrip import batch_of
from test_jpeg_decode_host import GREY, NAMES, file_of, fixture, gpu_vectors
from test_jpeg_roundtrip_host import COLOUR_SHAPES, GREY_SHAPES

pytestmark = pytest.mark.gpu

J = importlib.import_module("3d-magic-mirror_amd.jpeg")
JD = importlib.import_module("3d-magic-mirror_amd.jpeg_decode")
IB = importlib.import_module("3d-magic-mirror_amd.input_batches")

try:
    from PIL import Image
except ImportError:
    Image = None


def want_of(name, mode="RGB"):
    return torch.from_numpy(fixture()[("rgb_" if mode == "RGB" else "l_") + name])


def check_batch(names, mode="RGB", **kw):
    got = JD.decode_jpeg([file_of(n) for n in names], mode=mode, device=DEV, **kw)
    assert got.status.cpu().tolist() == [0] * len(names)
    assert len(got) == len(names) and got.images.dtype == torch.uint8 and got.images.dim() == 1
    for f, n in zip(got.frames, names):
        assert torch.equal(f.cpu(), want_of(n, mode)), n
    return got


def test_every_fixture_file_alone():
    for n in NAMES:
        check_batch([n])
    for n in GREY:
        check_batch([n], "L")


@pytest.mark.parametrize("order", ("forward", "reversed"))
def test_mixed_sizes_in_one_call(order):
    names = NAMES if order == "forward" else NAMES[::-1]
    got = check_batch(names)
    sizes = np.array([fixture()["rgb_" + n].shape[:2] for n in names])
    assert np.array_equal(got.sizes, sizes) and np.array_equal(got.offsets, np.concatenate([[0], np.cumsum(sizes[:, 0] * sizes[:, 1])]))
    assert got.images.numel() == 3 * got.offsets[-1]
    with pytest.raises(ValueError, match="different sizes"):
        got.stack()
    check_batch(GREY if order == "forward" else GREY[::-1], "L")


@pytest.mark.parametrize("layout", ("4:2:0", "4:2:2", "4:4:4", "L"))
def test_closed_loop_with_the_encoder_and_the_round_trip(layout):
    mode = "L" if layout == "L" else "RGB"
    for H, W in (GREY_SHAPES if mode == "L" else COLOUR_SHAPES):
        x = to_dev(batch_of(H, W, mode))
        for q in (100, 30):
            kw = {} if mode == "L" else {"subsampling": layout}
            files = J.encode_jpeg(x, q, mode, **kw)
            want = J.jpeg_roundtrip(x, q, mode, **kw)
            got = JD.decode_jpeg(files, mode=mode, device=DEV)
            assert torch.equal(got.stack(), want), (layout, H, W, q)
            assert not got.status.any()
            if mode == "L" and (H, W) == GREY_SHAPES[-1]:                        # a greyscale file in mode RGB replicates its plane
                rgb = JD.decode_jpeg(files, device=DEV).stack()
                assert torch.equal(rgb, want[..., None].expand(-1, -1, -1, 3))


def test_files_and_out_at_every_byte_alignment():
    shapes = ((1, 1), (3, 2), (5, 7), (2, 3), (1, 2))
    rng = np.random.default_rng(4)
    files, want = [], []
    for i, (H, W) in enumerate(shapes):
        x = to_dev(torch.from_numpy(rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)))
        s = ("4:2:0", "4:2:2", "4:4:4")[i % 3]
        files.append(J.encode_jpeg(x, 90, subsampling=s)[0])
        want.append(J.jpeg_roundtrip(x, 90, subsampling=s).reshape(-1))
    want = torch.cat(want)
    starts = np.cumsum([0] + [3 * h * w for h, w in shapes])[:-1]
    assert set(int(s) % 4 for s in starts) == {0, 1, 2, 3}
    for lead in range(4):
        storage = torch.full((want.numel() + 8,), 0xA5, dtype=torch.uint8, device=DEV)
        out = storage[lead:lead + want.numel()]
        assert out.data_ptr() % 4 == lead
        got = JD.decode_jpeg(files, device=DEV, out=out)
        assert got.images.data_ptr() == out.data_ptr() and torch.equal(out, want), lead
        assert (storage[:lead] == 0xA5).all() and (storage[lead + want.numel():] == 0xA5).all()      # nothing outside out is written
    for bad in (torch.empty(want.numel() + 1, dtype=torch.uint8, device=DEV), torch.empty(want.numel(), dtype=torch.int8, device=DEV),
                torch.empty(2 * want.numel(), dtype=torch.uint8, device=DEV)[::2]):
        with pytest.raises(ValueError, match="out must be"):
            JD.decode_jpeg(files, device=DEV, out=bad)


def test_257_files_span_the_grids():
    x = to_dev(torch.from_numpy(np.random.default_rng(257).integers(0, 256, (257, 8, 8, 3), dtype=np.uint8)))
    got = JD.decode_jpeg(J.encode_jpeg(x, 75), device=DEV)
    assert got.stack().shape == (257, 8, 8, 3) and torch.equal(got.stack(), J.jpeg_roundtrip(x, 75))


def test_256_noise_with_and_without_restart_rows():
    z = np.load(os.path.join(GOLDEN, "jpeg_decode_256.npz"))
    plain, rst = bytes(z["file_noise_256"]), bytes(z["file_noise_256_rstrow"])
    low = JD.lower_jpeg_decode([plain, rst])
    assert (low["segments"][:, JD.S_COUNT] > 0).sum() == 1 + 16
    got = JD.decode_jpeg([plain, rst], device=DEV)
    assert torch.equal(got.frames[0], got.frames[1])
    assert torch.equal(got.frames[0].cpu(), torch.from_numpy(z["rgb_noise_256"]))
    if Image is not None:
        assert torch.equal(got.frames[1].cpu(), torch.from_numpy(np.array(Image.open(io.BytesIO(rst)).convert("RGB"))))


def test_table_sets_are_grouped_and_results_keep_input_order():
    names = ["std_420_q75_17x23", "opt_420_q90_31x18", "market_128x64_q95", "opt_444_q60_9x9_noise", "one_pixel", "grey_opt_rst3_33x17", "std_422_q85_16x33"]
    low = JD.lower_jpeg_decode([file_of(n) for n in names])
    live = low["segments"][low["segments"][:, JD.S_COUNT] > 0]
    assert len(low["sets"]) >= 4 and live[0, JD.S_FILE] == 0 and not (np.diff(live[:, JD.S_FILE]) >= 0).all()      # the segments are reordered ...
    check_batch(names)                                                                                               # ... the frames are not


def test_image_pool_from_jpeg_then_assemble_batch():
    names = [n for n in NAMES if n != "one_pixel"]
    rng = np.random.default_rng(9)
    arrays = [fixture()["rgb_" + n] for n in names]
    segs = [(rng.random(a.shape[:2]) < 0.7).astype(np.uint8) * 255 for a in arrays]
    ref = IB.ImagePool(arrays, segs, DEV)
    pool = IB.ImagePool.from_jpeg([file_of(n) for n in names], segs, DEV)
    assert torch.equal(pool.buffer, ref.buffer)
    assert np.array_equal(pool.sizes, ref.sizes) and np.array_equal(pool.offsets, ref.offsets) and pool.sizes.dtype == ref.sizes.dtype
    for attr in ("images", "segs", "offsets_dev", "sizes_dev"):
        a, b = getattr(pool, attr), getattr(ref, attr)
        assert a.dtype == b.dtype and a.shape == b.shape and a.data_ptr() - pool.buffer.data_ptr() == b.data_ptr() - ref.buffer.data_ptr(), attr
    idx = list(range(len(names)))
    aug = IB.draw_augmentation("cub", pool.sizes[idx], rng=__import__("random").Random(3))
    assert torch.equal(IB.assemble_batch(pool, idx, (32, 32), "cub", aug), IB.assemble_batch(ref, idx, (32, 32), "cub", aug))
    with pytest.raises(ValueError, match="image 1"):
        IB.ImagePool.from_jpeg([file_of(n) for n in names], [segs[0], segs[0]] + segs[2:], DEV)


def test_zz_damaged_streams_return_status_and_the_host_decoders_pixels():
    """(last in the file: the vectors are forms the sanitized host program has decoded clean, tests/test_jpeg_decode_host.py)"""
    vectors = gpu_vectors() + [file_of("std_420_q75_17x23")]
    frames, status = JD.decode_jpeg_host(vectors)
    assert status.tolist() == [JD.ST_OVERRUN] * 3 + [JD.ST_BAD_CODE, 0]
    got = JD.decode_jpeg(vectors, device=DEV, strict=False)
    assert got.status.cpu().tolist() == status.tolist()
    for i, (g, w) in enumerate(zip(got.frames, frames)):
        assert torch.equal(g.cpu(), torch.from_numpy(w)), i
    with pytest.raises(ValueError, match=r"file 0: OVERRUN.*file 3: BAD_CODE"):
        JD.decode_jpeg(vectors, device=DEV)
