"""The JPEG file decoder on the MI355X on files that other encoders write (tests/golden/jpeg_foreign.npz; tests/jpeg_writer.py made them,
tests/test_jpeg_foreign_host.py proves by census what each holds): rearranged and redefined header segments, swapped table ids, every
selector pattern, Huffman codes of 10 to 16 bits in every table class, DC category 11, AC size 10, ZRL chains, blocks without EOB, 60 restart
intervals in one file.  ``torch.equal`` of every frame with the pixels Pillow read back, status all zero, sizes and offsets as lowered: no
tolerance, both sides are integer arithmetic.  The fixture alone is read: no Pillow is needed here.

Alone, every file's table set is its own and its luma always reads the set's first tables; in one call the tables are deduplicated over the
batch and the selector words change with the order, so the set runs forward, reversed, and interleaved with the Pillow-written files of
test_gpu_jpeg_decode.py.  The damaged vectors (BAD_RUN, BAD_SIZE) are forms the sanitized host program has passed, and they run last."""
import importlib

import numpy as np
import pytest
import torch

from test_gpu_export import DEV
from test_jpeg_decode_host import NAMES as PILLOW_NAMES, file_of as pillow_file_of, fixture as pillow_fixture
from test_jpeg_foreign_host import GREY, NAMES, file_of, fixture, gpu_vectors

pytestmark = pytest.mark.gpu

JD = importlib.import_module("3d-magic-mirror_amd.jpeg_decode")


def check_batch(items, mode="RGB"):
    """items: (file, the pixels wanted) pairs, decoded in one call"""
    files = [f for f, _ in items]
    low = JD.lower_jpeg_decode(files, mode)
    got = JD.decode_jpeg(files, mode=mode, device=DEV)
    assert got.status.cpu().tolist() == [0] * len(files)
    assert len(got) == len(files) and got.images.dtype == torch.uint8 and got.images.dim() == 1
    shapes = np.array([w.shape[:2] for _, w in items])
    assert np.array_equal(got.sizes, shapes) and np.array_equal(got.sizes, low["sizes"])
    assert np.array_equal(got.offsets, np.concatenate([[0], np.cumsum(shapes[:, 0] * shapes[:, 1])])) and np.array_equal(got.offsets, low["offsets"])
    assert got.images.numel() == low["channels"] * got.offsets[-1]
    for i, (f, (_, w)) in enumerate(zip(got.frames, items)):
        assert torch.equal(f.cpu(), torch.from_numpy(w)), i
    return low


def item(name, mode="RGB"):
    return file_of(name), fixture()[("rgb_" if mode == "RGB" else "l_") + name]


@pytest.mark.parametrize("name", NAMES)
def test_every_file_alone(name):
    check_batch([item(name)])
    if name in GREY:
        check_batch([item(name, "L")], "L")


@pytest.mark.parametrize("order", ("forward", "reversed"))
def test_all_in_one_call(order):
    names = NAMES if order == "forward" else NAMES[::-1]
    low = check_batch([item(n) for n in names])
    assert len(low["sets"]) >= 8 and (low["segments"][:, JD.S_COUNT] == 0).any()      # many table sets, their groups padded
    grey = GREY if order == "forward" else GREY[::-1]
    check_batch([item(n, "L") for n in grey], "L")


def test_interleaved_with_the_pillow_written_files():
    items = []
    for i in range(max(len(NAMES), len(PILLOW_NAMES))):
        if i < len(PILLOW_NAMES):
            items.append((pillow_file_of(PILLOW_NAMES[i]), pillow_fixture()["rgb_" + PILLOW_NAMES[i]]))
        if i < len(NAMES):
            items.append(item(NAMES[-1 - i]))
    low = check_batch(items)
    live = low["segments"][low["segments"][:, JD.S_COUNT] > 0]
    assert not (np.diff(live[:, JD.S_FILE]) >= 0).all()                                # the segments are regrouped by table set, the frames are not


def test_zz_bad_run_and_bad_size_return_status_and_the_host_decoders_pixels():
    """(last in the file: the vectors are forms the sanitized host program has decoded clean, tests/test_jpeg_foreign_host.py)"""
    vectors, want = gpu_vectors()
    frames, status = JD.decode_jpeg_host(vectors)
    assert status.tolist() == want == [JD.ST_BAD_RUN, JD.ST_BAD_RUN, JD.ST_BAD_SIZE, JD.ST_BAD_SIZE, 0]
    got = JD.decode_jpeg(vectors, device=DEV, strict=False)
    assert got.status.cpu().tolist() == status.tolist()
    for i, (g, w) in enumerate(zip(got.frames, frames)):
        assert torch.equal(g.cpu(), torch.from_numpy(w)), i
