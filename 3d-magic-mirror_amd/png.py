"""Device frames as PNG files, lossless: host side of ``mm_png_encode`` (csrc/mm_png.hip).

PNG is what the reference writes most: twelve ``vutils.save_image(..., '.png')`` sheets and two ``texure_maps.save(..., 'PNG')`` texture
maps per sample epoch (trainer.py:564-607), the ``*_single_img.py``, ``show_camera.py`` and ``show_rainbow2.py`` outputs, and every mask
the evaluation loop reads back (trainer.py:793,933).  ``encode_png`` takes the uint8 frames that ``export_images`` and ``export_grid`` leave
on the device -- (...,H,W,3) colour, (...,H,W) masks, (...,H,W,4) with alpha -- and returns the complete files, back to back in one host
buffer, after two device-to-host copies: the offsets, then exactly the bytes used.

The file is this project's own and fully specified, so it is held to a restatement byte for byte (tests/test_png_host.py), and to Pillow's
decoder for what it means: ``np.asarray(Image.open(file))`` equals the frame, to the bit.  Per frame: signature, IHDR, ONE IDAT, IEND.
Rows are filtered (per row the type of the least sum of absolute residuals, or one forced type), the filtered stream is cut into segments
of ``PNG_SEGMENT`` bytes, and each segment is one deflate block with the fixed Huffman codes whose matches never reach before the segment
-- which is what lets the coder run in parallel (and what makes the files larger than a serial coder's with dynamic codes).  No floating
point anywhere; the order is in DESIGN.md and in the kernel's header.

Out of scope: dynamic Huffman codes and stored blocks, matches across segments, lazy matching, interlacing, palettes, 16-bit depth,
ancillary chunks, APNG, Pillow's or libpng's own bytes, ``save_image(normalize=True)``'s min-max stretch, ``bench.py``.  Decoding -- these
files and other encoders' -- is ``decode_png`` in png_decode.py.
Device tensors only."""
import functools

import numpy as np
import torch

from . import _native as N
from .jpeg import JpegBatch

PNG_SEGMENT = N.PNG_SEGMENT              # MM_PNG_SEGMENT: bytes of the filtered stream that share a match window (tools/bench_png.py measured 1024, 2048, 4096)
PNG_MAX_SEGMENT = N.PNG_MAX_SEGMENT      # MM_PNG_MAX_SEGMENT: a segment's bytes and its table of 16-bit positions fit 64 KiB of LDS
PNG_CRC_PIECE = N.PNG_CRC_PIECE          # MM_PNG_CRC_PIECE: bytes of an IDAT whose CRC one lane takes
MAX_FRAMES = 65535                       # frames in a call
MAX_IDAT = (1 << 31) - 1                 # a chunk's length
MAX_SEGMENTS = (1 << 31) - 1             # segments in a call: a launch's grid

MODES = {"L": (1, 0), "RGB": (3, 2), "RGBA": (4, 6)}          # mode -> (channels, colour type)
_LAYOUT = {"L": "(...,H,W)", "RGB": "(...,H,W,3)", "RGBA": "(...,H,W,4)"}
_ADVICE = {"L": "export_images(x, 'mask') makes 8-bit masks", "RGB": "export_images makes 8-bit frames", "RGBA": "export_images(x, 'rgba') makes 8-bit frames"}


class PngBatch(JpegBatch):
    """n complete PNG files back to back in one host uint8 buffer; file i is ``buffer[offsets[i]:offsets[i + 1]]``.  ``JpegBatch``'s
    interface: ``len``, ``[i]``, iteration, ``write(paths)``, ``buffer``, ``offsets``, ``shape``"""


def check_mode(mode):
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError("mode must be 'RGB', 'L' or 'RGBA', got %r" % (mode,))
    return MODES[mode]


def check_segment(segment):
    segment = PNG_SEGMENT if segment is None else segment
    if isinstance(segment, bool) or not isinstance(segment, (int, np.integer)) or segment < 1 or segment > PNG_MAX_SEGMENT:
        raise ValueError("segment must be an int in 1..%d, got %r" % (PNG_MAX_SEGMENT, segment))
    return int(segment)


def check_filter(filter):
    """the filter as MMPngDesc wants it: -1 for "adaptive", or the forced type 0..4"""
    if isinstance(filter, str) and filter == "adaptive":
        return -1
    if isinstance(filter, bool) or not isinstance(filter, (int, np.integer)) or filter < 0 or filter > 4:
        raise ValueError("filter must be 'adaptive' or an int in 0..4 (None, Sub, Up, Average, Paeth), got %r" % (filter,))
    return int(filter)


@functools.lru_cache(maxsize=64)
def lower_png(H, W, mode="RGB", segment=None):
    """A frame size, mode and segment length as the sizes the kernels go by (host arithmetic only; nothing is launched): a dict of
    channels and colour_type; row_bytes, a filtered row (1 + W * channels); stream_bytes, the filtered stream S of one frame; segs, its
    segments; slot_words, the 32-bit words kept for one segment's bits (3 + 9 * segment + 7: the exact worst case, a match never costs
    more than its bytes as literals); deflate_capacity, idat_capacity and file_capacity, the most bytes a frame's deflate blocks, IDAT
    data and file take (8 + 25 + 12 + (2 + ceil(sum over segments of (10 + 9 len) / 8) + 4) + 12); and ``workspace_bytes(n)`` /
    ``files_offset(n)``, what n frames need and where their files start in it: mm_png_query_workspace and mm_png_files_offset in Python.
    The dict is cached and shared between calls: read, not written.  ValueError for what the kernel refuses."""
    channels, colour_type = check_mode(mode)
    segment = check_segment(segment)
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H > 65535 or W > 65535:
        raise ValueError("a PNG frame here is 1..65535 pixels each way, got %d x %d" % (H, W))
    row = 1 + W * channels
    stream = row * H
    segs = (stream + segment - 1) // segment
    frame_bits = 10 * segs + 9 * stream
    deflate = (frame_bits + 7) // 8
    if 2 + deflate + 4 > MAX_IDAT:
        raise ValueError("the IDAT of a %d x %d %s frame could take %d bytes, more than 2**31 - 1" % (H, W, mode, 2 + deflate + 4))
    slot_words = (10 + 9 * segment + 31) // 32
    raw_words = (frame_bits + 31) // 32 + 1
    low = dict(H=H, W=W, mode=mode, segment=segment, channels=channels, colour_type=colour_type, row_bytes=row, stream_bytes=stream, segs=segs,
               slot_words=slot_words, deflate_capacity=deflate, idat_capacity=2 + deflate + 4, file_capacity=8 + 25 + 12 + (2 + deflate + 4) + 12)
    up = N.up256
    # offsets (n + 1) int64 | the files | the packed streams | a CRC word per frame | bits and Adler-32 per frame | bits per segment |
    # Adler sums per segment | S | a slot per segment
    low["files_offset"] = lambda n: up((n + 1) * 8)
    low["workspace_bytes"] = lambda n: (up((n + 1) * 8) + up(n * low["file_capacity"]) + up(n * raw_words * 4) + up(n * 4) + up(n * 16)
                                        + 2 * up(n * segs * 8) + up(n * stream) + up(n * segs * slot_words * 4))
    return low


def check_frames(frames, mode="RGB", filter="adaptive", segment=None):
    """the argument errors of ``encode_png``, before anything touches a device: (n, lead, low, filter as MMPngDesc wants it)"""
    channels, _ = check_mode(mode)
    filter = check_filter(filter)
    segment = check_segment(segment)
    layout = _LAYOUT[mode]
    if not torch.is_tensor(frames):
        raise ValueError("frames must be a uint8 tensor %s, got %s" % (layout, type(frames)))
    if frames.dtype != torch.uint8:
        raise ValueError("frames must be uint8 %s, got %s: %s from float renders" % (layout, frames.dtype, _ADVICE[mode]))
    lead = frames.dim() - (2 if mode == "L" else 3)              # the leading dimensions
    if lead < 0 or (mode != "L" and frames.shape[-1] != channels):
        raise ValueError("frames of mode %r must have shape %s, got %s" % (mode, layout, tuple(frames.shape)))
    if min(frames.shape, default=1) < 1:
        raise ValueError("an empty batch: frames of shape %s" % (tuple(frames.shape),))
    n = int(np.prod(frames.shape[:lead], dtype=np.int64))
    if n > MAX_FRAMES:
        raise ValueError("at most %d frames in a call, got shape %s" % (MAX_FRAMES, tuple(frames.shape)))
    H, W = (int(v) for v in frames.shape[lead:lead + 2])
    low = lower_png(H, W, mode, segment)
    if n * low["segs"] > MAX_SEGMENTS:
        raise ValueError("%d frames of %d segments each: more than 2**31 - 1 segments in a call" % (n, low["segs"]))
    return n, tuple(frames.shape[:lead]), low, filter


def encode_png(frames, mode="RGB", filter="adaptive", segment=None):
    """Frames as PNG files, 8 bits per sample, lossless: a ``PngBatch``.  ``np.asarray(PIL.Image.open(file))`` is the frame, to the bit.

    frames       device uint8: (...,H,W,3) for mode "RGB", what ``export_grid`` and ``export_images`` return; (...,H,W) for "L", what
                 ``export_images(x, "mask")`` returns; (...,H,W,4) for "RGBA", ``export_images(x, "rgba")``.  Any byte alignment; other
                 strides go through ``.contiguous()``.  Float input is refused: ``export_images`` makes the bytes.
    mode         "RGB", "L" or "RGBA": colour type 2, 0 or 6
    filter       "adaptive": per row the filter type whose residuals have the least sum of absolute values (ties: the lowest type); or an
                 int 0..4 that forces None, Sub, Up, Average or Paeth on every row
    segment      bytes of the filtered stream that share a match window, 1..``PNG_MAX_SEGMENT``; None is ``PNG_SEGMENT``.  Smaller
                 segments code faster and compress less.

    ``batch[i]`` is file i as bytes, ``batch.write(paths)`` writes them, ``batch.shape`` keeps the leading dimensions (files are in
    row-major order over them).  Nothing synchronises until the end; then two device-to-host copies: the n + 1 offsets, then exactly the
    bytes used.  ``batch.buffer`` is pinned host memory and stays allocated for as long as the batch is held.  ValueError, before anything
    touches a device: another dtype or channel count than the mode's, an empty batch, H or W outside 1..65535, an unknown mode or filter, a
    segment out of range, a frame whose IDAT could exceed 2**31 - 1 bytes, more than 65535 frames or 2**31 - 1 segments in a call.

    The files are larger than a serial encoder's with dynamic Huffman codes (DESIGN.md has the sizes); that is the price of coding the
    segments independently.  Out of scope: see the module's docstring.

        encode_png(export_grid(x, rounding="nearest")).write([path])      # was: vutils.save_image(x, path, nrow=8, padding=2)
        encode_png(export_images(tex)).write(names)                       # was: per map to_pil_image(...).save(name, 'PNG')
        encode_png(export_images(x, "mask"), "L").write(mask_names)       # was: per mask save_image(mask, name)"""
    n, lead, low, filter = check_frames(frames, mode, filter, segment)
    N.require_device(frames)
    x = frames.detach().contiguous()
    dev = x.device
    d = N.MMPngDesc()
    d.n, d.H, d.W, d.channels, d.filter, d.segment = n, low["H"], low["W"], low["channels"], filter, low["segment"]
    d.frames = N.ptr(x)
    ws = N.checked_workspace("mm_png_query_workspace", d, dev, (low["workspace_bytes"](n), low["files_offset"](n)), ("mm_png_files_offset",),
                             lambda got, want: "mm_png_query_workspace gives %s (bytes, where the files start), lower_png %s" % (got, want))
    N.call("mm_png_encode", dev, d)
    off, buf = N.read_back(ws, n + 1, low["files_offset"](n))            # two blocking copies: the n + 1 offsets, exactly the bytes used
    return PngBatch(buf, off, lead)
