"""Device frames as one animated GIF file: host side of ``mm_gif_encode`` (csrc/mm_gif.hip).

The reference's signature output is the turntable GIF, and every script writes it the same way: ``imageio.get_writer(path, mode='I')`` and a
loop of render -> ``make_grid`` -> ``.cpu()`` -> ``(image * 255).astype(np.uint8)`` -> ``writer.append_data(image)`` (trainer.py:616-695,
show_rainbow2.py:377-470, show_camera.py:396-500, CUB_ / MKT_ / THU_single_img.py:372-390).  ``encode_gif`` takes the (n,H,W,3) uint8 frames
that ``export_grid``, ``export_images``, ``composite_frames`` and ``pyramid_frames`` leave on the device and returns the complete file in
one host buffer after two device-to-host copies: its length, then exactly the bytes used.

The file is this project's own and fully specified, so it is held to a restatement byte for byte (tests/test_gif_host.py), and to Pillow's
decoder for what it means.  One global palette of 256 colours from a median cut over a 15-bit histogram of ALL frames of the call; a pixel's
index is the box of its histogram bin; LZW in independent segments of ``GIF_SEGMENT`` pixels, each with a fresh dictionary, which is what
lets the coder run in parallel (and what makes the files larger than a serial coder's).  No floating point anywhere; the order is in
DESIGN.md and in the kernel's header.

``delay=10, loop=0`` are what imageio's ``mode='I'`` GIF writer is remembered to default to (0.1 s per frame, loop forever): recalled, not
checked -- imageio is not installed here and was never run against.

Out of scope: per-frame local palettes, caller-supplied palettes, dithering, transparency, disposal tricks and frame differencing,
Pillow's or imageio's own bytes (neither is a target), decoding, ``bench.py``.  Device tensors only."""
import numpy as np
import torch

from . import _native as N

GIF_SEGMENT = N.GIF_SEGMENT          # MM_GIF_SEGMENT: pixels that share an LZW dictionary (tools/bench_gif.py measured 512, 1024 and 2048)
MAX_SEGMENT = N.GIF_MAX_SEGMENT      # MM_GIF_MAX_SEGMENT: 257 + 3838 = 4095, the dictionary can never fill
MAX_PIXELS = 1 << 29                 # n*H*W of a call stays below this: 7 * count fits 32 bits
MAX_FRAMES = 65535
FILE_OFFSET = 256                    # mm_gif_file_offset


def worst_bits(length):
    """the most bits a segment of ``length`` pixels codes to: length + 1 codes, every data code new, code k at
    9 + (k >= 255) + (k >= 767) + (k >= 1791) bits"""
    codes = length + 1
    return 9 * codes + max(codes - 255, 0) + max(codes - 767, 0) + max(codes - 1791, 0)


def workspace_bytes(n, H, W, segment=GIF_SEGMENT, loop=0, quantize_only=False):
    """mm_gif_query_workspace in Python: length | file | histogram | table | packed streams | bit offsets | frame offsets and bits | slots"""
    up = N.up256
    if quantize_only:
        return 256 + 32768 * 17
    pixels = H * W
    segs = (pixels + segment - 1) // segment
    slot_words = (worst_bits(segment) + 9 + 31) // 32 + 1
    frame_bits = 9 + (segs - 1) * worst_bits(segment) + worst_bits(pixels - (segs - 1) * segment)
    raw_words = (frame_bits + 31) // 32 + 1
    stream = (frame_bits + 7) // 8
    file_cap = 13 + 768 + (19 if loop is not None else 0) + n * (20 + stream + (stream + 254) // 255) + 1
    return (256 + up(file_cap) + 32768 * 17 + up(n * raw_words * 4) + up(n * segs * 8) + up((2 * n + 1) * 8) + up(n * segs * slot_words * 4))


class GifFile:
    """one complete GIF file in a host uint8 buffer: ``bytes(g)``, ``len(g)``, ``g.write(path)``, ``g.palette`` (256,3) uint8"""

    def __init__(self, buffer):
        self.buffer = buffer
        self._view = memoryview(buffer.numpy() if torch.is_tensor(buffer) else np.asarray(buffer))

    def __len__(self):
        return len(self._view)

    def __bytes__(self):
        return bytes(self._view)

    @property
    def palette(self):
        return np.frombuffer(self._view[13:13 + 768], dtype=np.uint8).reshape(256, 3).copy()

    def write(self, path):
        with open(path, "wb") as f:
            f.write(self._view)


def check_frames(frames):
    """the argument errors of ``quantize_frames`` and ``encode_gif`` about the frames, before anything touches a device: (n, H, W)"""
    if not torch.is_tensor(frames):
        raise ValueError("frames must be a uint8 tensor (n,H,W,3) or (H,W,3), got %s" % type(frames))
    if frames.dtype != torch.uint8:
        raise ValueError("frames must be uint8 (n,H,W,3), got %s: export_images makes 8-bit frames from float renders" % frames.dtype)
    if frames.dim() not in (3, 4) or frames.shape[-1] != 3:
        raise ValueError("frames must have shape (n,H,W,3) or (H,W,3), got %s" % (tuple(frames.shape),))
    if min(frames.shape) < 1:
        raise ValueError("an empty batch: frames of shape %s" % (tuple(frames.shape),))
    n = int(frames.shape[0]) if frames.dim() == 4 else 1
    H, W = (int(v) for v in frames.shape[-3:-1])
    if H > 65535 or W > 65535:
        raise ValueError("a GIF frame is 1..65535 pixels each way, got %d x %d" % (H, W))
    if n > MAX_FRAMES:
        raise ValueError("at most %d frames in a call, got %d" % (MAX_FRAMES, n))
    if n * H * W >= MAX_PIXELS:
        raise ValueError("n*H*W must stay below 2**29 (the histogram's 32-bit sums), got %d x %d x %d" % (n, H, W))
    return n, H, W


def check_timing(n, delay, loop):
    """the argument errors about delay and loop: (delay as an int, or a list of n ints; loop as an int, -1 for None)"""
    def one(v, what, lo):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or v > 65535:
            raise ValueError("%s must be an int in %d..65535, got %r" % (what, lo, v))
        return int(v)
    if isinstance(delay, (int, np.integer)) and not isinstance(delay, bool):
        delay = one(delay, "delay (centiseconds)", 0)
    else:
        try:
            delay = list(delay)
        except TypeError:
            raise ValueError("delay must be an int in 0..65535 or a sequence of n of them, got %r" % (delay,))
        if len(delay) != n:
            raise ValueError("%d delays for %d frames" % (len(delay), n))
        delay = [one(v, "delay (centiseconds)", 0) for v in delay]
    return delay, -1 if loop is None else one(loop, "loop", 0)


def _launch(frames, n, H, W, segment, delay, loop, quantize_only):
    x = frames.detach().contiguous()
    dev = x.device
    palette = torch.empty((256, 3), dtype=torch.uint8, device=dev)
    indices = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    d = N.MMGifDesc()
    d.n, d.H, d.W, d.segment, d.loop, d.quantize_only = n, H, W, segment, loop, int(quantize_only)
    d.frames, d.palette, d.indices = N.ptr(x), N.ptr(palette), N.ptr(indices)
    keep = None
    if isinstance(delay, list):
        keep = N.upload_int32(np.asarray(delay, dtype=np.int32), dev)
        d.delays = N.ptr(keep[1])
    else:
        d.delay = delay
    want = (workspace_bytes(n, H, W, segment, None if loop < 0 else loop, quantize_only),) + (() if quantize_only else (FILE_OFFSET,))
    ws = N.checked_workspace("mm_gif_query_workspace", d, dev, want, ("mm_gif_file_offset",)[:len(want) - 1],
                             lambda got, want: "mm_gif_query_workspace gives %d bytes, gif.workspace_bytes %d" % (got[0], want[0]))
    N.call("mm_gif_encode", dev, d)
    del keep                                                             # (the allocator keeps it for the stream until the kernels are through)
    return palette, indices, ws


def quantize_frames(frames):
    """The first half of ``encode_gif``: ``(palette, indices)``, (256,3) uint8 and (n,H,W) uint8, both on the device; ``palette[indices]``
    are the frames as the file shows them.  One palette for all frames of the call: a median cut over the non-empty bins of the 15-bit
    histogram (count-weighted median along the widest axis, ties g, r, b; the box with the most pixels first), each entry the rounded mean
    of its box, unused entries 0,0,0; a pixel's index is the box of its bin.  Nothing synchronises.  ValueError as ``encode_gif``."""
    n, H, W = check_frames(frames)
    N.require_device(frames)
    palette, indices, _ = _launch(frames, n, H, W, GIF_SEGMENT, 0, -1, True)
    return palette, indices


def encode_gif(frames, delay=10, loop=0, segment=None):
    """Frames as one animated GIF89a file: a ``GifFile``.

    frames       device uint8 (n,H,W,3), what ``export_grid``, ``export_images``, ``composite_frames`` and ``pyramid_frames`` return; a single
                 (H,W,3) frame is n = 1; any byte alignment; other strides go through ``.contiguous()``.  Float input is refused:
                 ``export_images`` makes the bytes.
    delay        centiseconds per frame, an int or a sequence of n ints, each in 0..65535
    loop         the NETSCAPE2.0 loop count (0: forever), or None to leave the extension out
    segment      pixels that share an LZW dictionary, 1..3838; None is ``GIF_SEGMENT``.  Smaller segments code faster and compress less.

    ``delay=10, loop=0`` are what imageio's ``mode='I'`` writer is remembered to default to; imageio was never run against (see the module's
    docstring).  ``bytes(g)`` is the file, ``g.write(path)`` writes it, ``g.palette`` is its colour table.  Nothing synchronises until the
    end; then two device-to-host copies, the length and exactly the bytes used.  ``g.buffer`` is pinned host memory.  ValueError: another
    dtype or channel count, an empty batch, H or W above 65535, n*H*W >= 2**29, a delay or loop outside 0..65535.

    Out of scope: local palettes, caller-supplied palettes, dithering, transparency, disposal tricks, frame differencing, Pillow's or
    imageio's own bytes, decoding.

        sheet = export_grid(render_views(...)[0], nrow=8)                 # (36,Hg,Wg,3) uint8, on the device
        encode_gif(sheet).write(path)                                     # was: per view .cpu() ... writer.append_data(image)"""
    n, H, W = check_frames(frames)
    delay, loop = check_timing(n, delay, loop)
    segment = GIF_SEGMENT if segment is None else segment
    if isinstance(segment, bool) or not isinstance(segment, (int, np.integer)) or segment < 1 or segment > MAX_SEGMENT:
        raise ValueError("segment must be an int in 1..%d, got %r" % (MAX_SEGMENT, segment))
    N.require_device(frames)
    _, _, ws = _launch(frames, n, H, W, int(segment), delay, loop, False)
    return GifFile(N.read_back(ws, 1, FILE_OFFSET)[1])                    # two blocking copies: the file's length, exactly the bytes used
