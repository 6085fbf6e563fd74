"""The PNG decoder's row of the stream-order table (tests/stream_order.py), added from here.

tests/stream_order.py keeps one ``Case`` per operator and its census (tests/test_stream_order_host.py) wants a case for every export that
takes a stream.  ``mm_png_decode`` is such an export; its case is appended to ``stream_order.CASES`` when this module is imported, which
the PNG decoder's two test files do -- both are collected before the stream-order files, so the census, the decoy check and the
delayed-side-stream test of tests/test_gpu_stream_order.py run it with the other operators' cases."""
import numpy as np
import torch

import png_writer as PW
import stream_order as SO

NAME = "decode_png (strict=False, out=)"


def png_files():
    """three small files of different colour types, depths and sizes, written by tests/png_writer.py (no Pillow needed)"""
    def make():
        r = np.random.default_rng(46)
        return [PW.png_of(r.integers(0, 256, (5, 7, 3)).astype(np.uint8), 8, 2, (4, 1, 3)),
                PW.png_of(r.integers(0, 4, (9, 6)).astype(np.uint8), 2, 0, (2, 0)),
                PW.png_of(r.integers(0, 256, (3, 4, 4)).astype(np.uint8), 8, 6, (3,))]
    return SO.once("png_files", make)


def decode_png_inputs(seed):
    low = SO.mod("png_decode").lower_png_decode(png_files(), "RGB")
    return (torch.from_numpy(SO.rng_of(seed).integers(0, 256, 3 * int(low["offsets"][-1]), dtype=np.uint8)),)


def decode_png_op(out):
    got = SO.mod("png_decode").decode_png(png_files(), "RGB", out=out, strict=False)
    assert got.images.data_ptr() == out.data_ptr()
    return [got.images, got.status]


def check_decode_png(out):
    low = SO.mod("png_decode").lower_png_decode(png_files(), "RGB")
    assert out.dtype == torch.uint8 and out.numel() == 3 * int(low["offsets"][-1])


CASE = SO.case(NAME, decode_png_inputs, decode_png_op, ("mm_png_decode",), check=check_decode_png)
if NAME not in SO.BY_NAME:
    SO.CASES.append(CASE)
    SO.BY_NAME[NAME] = CASE
