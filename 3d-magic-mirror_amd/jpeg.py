"""Device frames as baseline JPEG files, Pillow's bytes: host side of ``mm_jpeg_modes_encode`` (csrc/mm_jpeg.hip).

The reference's dataset-generation, evaluation and visualisation scripts all end on ``to_pil_image(X[i, :3].cpu())`` followed by
``output.save(name, 'JPEG', quality=100)`` (trainer.py:51, test.py:53, generate_market++.py:55, tool/generate_market_test.py:57, ...), one
image and one process at a time.  ``encode_jpeg`` takes the (...,H,W,3) uint8 frames that ``export_images``, ``composite_frames`` and
``pyramid_frames`` leave on the device and returns the complete files, back to back in one host buffer, after two device-to-host copies:
the offsets, then exactly the bytes used.  With ``mode="L"`` it takes the (...,H,W) masks of ``export_images(x, "mask")`` and writes
greyscale files (``to_pil_image(X[i, 3])``, the rec_mask / ori_mask files of trainer.py:697-769 and test.py:302-383).

Every file equals, byte for byte, what ``PIL.Image.fromarray(frame).save(f, 'JPEG', quality=q, subsampling=s)`` writes (Pillow 12 over
libjpeg-turbo): baseline, 4:2:0 (the default), 4:2:2 or 4:4:4, or greyscale; the standard Huffman tables, libjpeg's quality scaling.  libjpeg's baseline path is all integer and so is this one; the
order is in DESIGN.md and in the kernel's header.  The host makes the tables and the header (``lower_jpeg``); everything after SOS is
made on the device.

``jpeg_roundtrip`` is the other half of what the evaluation does: the frames as ``Image.open(file).convert('RGB')`` (and, for a mask,
``.convert('L')`` of its greyscale file) reads them back, to the byte, from the coefficients the encoder's transform leaves in memory --
host side of ``mm_jpeg_roundtrip``.

Out of scope: 4:1:1 and 4:4:0 subsampling, CMYK / RGBA, ``optimize=True``, progressive, restart markers, EXIF / ICC, writing to
disk beyond ``JpegBatch.write``.  The round trip of our own frames is ``jpeg_roundtrip``; decoding arbitrary files (marker parser, the
file's own tables, an entropy decoder, restart intervals) is ``decode_jpeg`` in jpeg_decode.py.  Device tensors only."""
import ctypes
import functools

import numpy as np
import torch

from . import _native as N

BLOCK_BYTES = 208       # MM_JPEG_BLOCK_BYTES: a block codes to at most 20 + 63 * 26 bits, kept as 52 words
CHUNK_BYTES = 1024      # MM_JPEG_CHUNK_BYTES: the piece of a stream one workgroup stuffs
MAX_BLOCKS = 1 << 20    # MM_JPEG_MAX_BLOCKS: blocks of one frame (its stream's bit offsets stay inside 31 bits)
MAX_FRAMES = 65535      # frames in a call

# ITU-T T.81 Annex K: the two base quantisation tables (natural order) and the four Huffman tables (codes per length 1..16, symbols)
_Q_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_Q_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
_AC_LUMA = ("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
            "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6"
            "c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = ("000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
              "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
              "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
# (class << 4 | id, bits, symbols) in the order the four DHT segments are written: DC 0, AC 0, DC 1, AC 1
HUFFMAN = ((0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),
           (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), bytes.fromhex(_AC_LUMA)),
           (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),
           (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), bytes.fromhex(_AC_CHROMA)))


def _zigzag():
    """ZIGZAG[k]: the natural (row-major) index of the k-th coefficient in zigzag order"""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) % 2 else i % 8))
    return np.array(order, dtype=np.int32)


ZIGZAG = _zigzag()


def quant_tables(quality):
    """(2,64) int32, natural order: the luma and chroma tables by libjpeg's ``jpeg_set_quality(quality, force_baseline=TRUE)``"""
    quality = int(quality)
    if quality < 1 or quality > 100:
        raise ValueError("quality must be an int in 1..100, got %r" % (quality,))
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    base = np.array([_Q_LUMA, _Q_CHROMA], dtype=np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.int32)


@functools.lru_cache(maxsize=None)
def huffman_codes():
    """(4,256) int32, ``size << 16 | code`` per symbol (0 where the table has none), tables in ``HUFFMAN``'s order: T.81 Annex C"""
    out = np.zeros((4, 256), dtype=np.int32)
    for t, (_, bits, vals) in enumerate(HUFFMAN):
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                out[t, vals[k]] = length << 16 | code
                code, k = code + 1, k + 1
            code <<= 1
    out.setflags(write=False)
    return out


def _segment(marker, body):
    return bytes((0xFF, marker)) + (len(body) + 2).to_bytes(2, "big") + body


SUBSAMPLINGS = ("4:4:4", "4:2:2", "4:2:0")        # Pillow's ints 0, 1, 2 in this order
# what an MCU is, per layout: (blocks, luma blocks across and down, of 8 x 8 pixels, Y's sampling byte in SOF0); JpegMcu in csrc/mm_jpeg_idct.h
MCU = {"4:2:0": (6, 2, 2, 0x22), "4:2:2": (4, 2, 1, 0x21), "4:4:4": (3, 1, 1, 0x11), "L": (1, 1, 1, 0x11)}
MODES = {"RGB": N.JPEG_MODE_RGB, "L": N.JPEG_MODE_L}
SAMPLINGS = {"4:2:0": N.JPEG_SAMPLING_420, "4:2:2": N.JPEG_SAMPLING_422, "4:4:4": N.JPEG_SAMPLING_444, "L": 0}      # by layout: MM_JPEG_SAMPLING_*


def plane_bytes(layout, mcus):
    """the bytes of the padded sample planes of one image of ``mcus`` MCUs, (Y, Cb and Cr together): JpegPlanes in csrc/mm_jpeg_idct.h"""
    per, lh, lv, _ = MCU[layout]
    return mcus * 64 * lh * lv, mcus * 64 * (per - lh * lv)


def check_layout(mode, subsampling="4:2:0"):
    """mode and subsampling as one key of ``MCU``: "L", or the subsampling as a string.  ValueError for an unknown mode or subsampling, and
    for a subsampling other than the default with mode "L" (a greyscale file has one component: there is nothing to subsample)"""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError("mode must be 'RGB' or 'L', got %r" % (mode,))
    if isinstance(subsampling, (int, np.integer)) and not isinstance(subsampling, bool) and 0 <= subsampling < 3:
        subsampling = SUBSAMPLINGS[subsampling]
    if not isinstance(subsampling, str) or subsampling not in SUBSAMPLINGS:
        raise ValueError("subsampling must be one of '4:4:4', '4:2:2', '4:2:0' (or Pillow's 0, 1, 2), got %r" % (subsampling,))
    if mode == "L":
        if subsampling != "4:2:0":
            raise ValueError("subsampling must stay at its default with mode 'L' (a greyscale file has one component), got %r" % (subsampling,))
        return "L"
    return subsampling


def header_bytes(H, W, qtables, layout="4:2:0"):
    """a file up to and including SOS, in Pillow's order: SOI, APP0 (JFIF 1.01, units 0, density 1 x 1), one DQT per table (zigzag order),
    SOF0 (Y 2x2, 2x1 or 1x1 by the layout, Cb 1x1, Cr 1x1), four DHT segments, SOS.  Layout "L": one DQT, one component, the two luma DHTs"""
    grey = layout == "L"
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(1 if grey else 2):
        out += _segment(0xDB, bytes((t,)) + bytes(int(v) for v in np.asarray(qtables)[t][ZIGZAG]))
    comps = b"\x01\x01\x11\x00" if grey else b"\x03\x01" + bytes((MCU[layout][3],)) + b"\x00\x02\x11\x01\x03\x11\x01"
    out += _segment(0xC0, b"\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big") + comps)
    for tc_th, bits, vals in HUFFMAN[:2] if grey else HUFFMAN:
        out += _segment(0xC4, bytes((tc_th,)) + bytes(bits) + vals)
    return out + _segment(0xDA, b"\x01\x01\x00\x00\x3f\x00" if grey else b"\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00")


def lower_jpeg(H, W, quality=100, mode="RGB", subsampling="4:2:0"):
    """A frame size, quality and layout as the tables the kernels read (host arithmetic only; nothing is launched): a dict of
    qtables (2,64) int32, natural order; divisors (2,64) int32 = 8 * q, natural order (the islow transform leaves its output scaled by 8);
    huffman (4,256) int32; header, the bytes up to and including SOS; mode, subsampling (a string; None in mode "L"); mcu_rows, mcu_cols,
    blocks_per_mcu (6 for 4:2:0, 4 for 4:2:2, 3 for 4:4:4, 1 for greyscale), mcu_height, mcu_width (pixels), blocks; stream_capacity, the bytes
    kept for one frame's entropy-coded data before stuffing (208 per block, in whole 1024-byte chunks); file_capacity, the most one file
    takes (header + twice that + EOI); ``params``, all of it packed as MMJpegDesc.params wants it (int32 words; the header's bytes in
    file order, padded to a word); and ``workspace_bytes(n)`` / ``files_offset(n)`` / ``coef_offset(n)``, what n frames need and where their
    files and coefficients start in it: mm_jpeg_query_workspace, mm_jpeg_files_offset and mm_jpeg_coef_offset in Python;
    ``roundtrip_workspace_bytes(n, mode="RGB", own_coef=True)``: mm_jpeg_roundtrip_query_workspace in Python (mode "RGB" of a greyscale
    dict is refused).  ``params`` holds both divisor tables and all four code tables in every layout; only the header differs.
    The dict is cached and shared between calls: read, not written.  ValueError for what the kernel refuses."""
    return _lower(int(H), int(W), quality, check_layout(mode, subsampling))


@functools.lru_cache(maxsize=32)
def _lower(H, W, quality, layout):
    if H < 1 or W < 1 or H > 65535 or W > 65535:
        raise ValueError("a JPEG frame is 1..65535 pixels each way, got %d x %d" % (H, W))
    q = quant_tables(quality)
    per_mcu, lh, lv, _ = MCU[layout]
    my, mx = (H + 8 * lv - 1) // (8 * lv), (W + 8 * lh - 1) // (8 * lh)
    blocks = my * mx * per_mcu
    if blocks > MAX_BLOCKS:
        raise ValueError("a frame of %d x %d has %d blocks, more than %d" % (H, W, blocks, MAX_BLOCKS))
    chunks = (blocks * BLOCK_BYTES + CHUNK_BYTES - 1) // CHUNK_BYTES
    header = header_bytes(H, W, q, layout)
    pad = -len(header) % 4
    params = np.concatenate([(8 * q).reshape(-1), huffman_codes().reshape(-1),
                             np.frombuffer(header + b"\0" * pad, dtype=np.uint8).view(np.int32)]).astype(np.int32)
    low = dict(H=H, W=W, quality=int(quality), mode="L" if layout == "L" else "RGB", subsampling=None if layout == "L" else layout, layout=layout,
               blocks_per_mcu=per_mcu, mcu_height=8 * lv, mcu_width=8 * lh, qtables=q, divisors=8 * q, huffman=huffman_codes(), header=header, mcu_rows=my, mcu_cols=mx,
               blocks=blocks, chunks=chunks, stream_capacity=chunks * CHUNK_BYTES, file_capacity=len(header) + 2 * chunks * CHUNK_BYTES + 2,
               params=torch.from_numpy(params))
    up = N.up256
    # offsets (n + 1) int64 | the files | coefficients (int16 x 64 per block) | bits per block | bits per frame | the unstuffed streams | 0xFF per chunk
    low["files_offset"] = lambda n: up((n + 1) * 8)
    low["coef_offset"] = lambda n: up((n + 1) * 8) + up(n * low["file_capacity"])
    # mm_jpeg_roundtrip's: coefficients (unless it decodes mm_jpeg_encode's) | Y planes, an MCU's pixels in bytes | Cb and Cr planes, 128; mode L uses none
    def roundtrip_workspace_bytes(n, mode="RGB", own_coef=True):
        if mode == "L":
            return 256
        if layout == "L":
            raise ValueError("a greyscale layout has no colour round trip")
        return (up(n * blocks * 128) if own_coef else 0) + sum(up(n * b) for b in plane_bytes(layout, my * mx))

    low["roundtrip_workspace_bytes"] = roundtrip_workspace_bytes
    low["workspace_bytes"] = lambda n: (up((n + 1) * 8) + up(n * low["file_capacity"]) + up(n * blocks * 128) + up(n * blocks * 4) + up(n * 4)
                                        + up(n * chunks * CHUNK_BYTES) + up(n * chunks * 4))
    return low


class JpegBatch:
    """n complete JPEG files back to back in one host uint8 buffer; file i is ``buffer[offsets[i]:offsets[i + 1]]``"""

    def __init__(self, buffer, offsets, shape=None):
        self.buffer, self.offsets = buffer, [int(o) for o in offsets]
        self.shape = (len(self.offsets) - 1,) if shape is None else tuple(shape)       # the frames' leading dimensions
        self._view = memoryview(buffer.numpy() if torch.is_tensor(buffer) else np.asarray(buffer))

    def __len__(self):
        return len(self.offsets) - 1

    def __getitem__(self, i):
        n = len(self)
        if not isinstance(i, (int, np.integer)):
            raise TypeError("a %s is indexed by an int, got %r" % (type(self).__name__, i))
        if i < -n or i >= n:
            raise IndexError("file %d of %d" % (i, n))
        i = int(i) % n
        return bytes(self._view[self.offsets[i]:self.offsets[i + 1]])

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def write(self, paths):
        """file i to paths[i]"""
        paths = list(paths)
        if len(paths) != len(self):
            raise ValueError("%d paths for %d files" % (len(paths), len(self)))
        for i, p in enumerate(paths):
            with open(p, "wb") as f:
                f.write(self._view[self.offsets[i]:self.offsets[i + 1]])


def check_frames(frames, quality, layout="(...,H,W,3)"):
    """the argument errors of ``encode_jpeg``, before anything touches a device: (n, H, W).  layout "(...,H,W)": the same for masks
    (``jpeg_roundtrip``'s mode "L")"""
    rgb = layout.endswith(",3)")
    if not torch.is_tensor(frames):
        raise ValueError("frames must be a uint8 tensor %s, got %s" % (layout, type(frames)))
    if frames.dtype != torch.uint8:
        raise ValueError("frames must be uint8 %s, got %s: %s from float renders"
                         % (layout, frames.dtype, "export_images makes 8-bit frames" if rgb else "export_images(x, 'mask') makes 8-bit masks"))
    lead = frames.dim() - (3 if rgb else 2)                               # the leading dimensions
    if lead < 0 or (rgb and frames.shape[-1] != 3):
        raise ValueError("frames must have shape %s, got %s" % (layout, tuple(frames.shape),))
    if min(frames.shape) < 1:
        raise ValueError("an empty batch: frames of shape %s" % (tuple(frames.shape),))
    n = int(np.prod(frames.shape[:lead], dtype=np.int64))
    if n > MAX_FRAMES:
        raise ValueError("at most %d frames in a call, got shape %s" % (MAX_FRAMES, tuple(frames.shape)))
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or quality < 1 or quality > 100:
        raise ValueError("quality must be an int in 1..100, got %r" % (quality,))
    H, W = frames.shape[lead:lead + 2]
    return n, int(H), int(W)


@functools.lru_cache(maxsize=16)
def _resident_params(device, H, W, quality, layout="4:2:0"):
    """``lower_jpeg``'s table in the device's memory, kept between calls (a run repeats one size, quality and layout).
    Resident: uploaded once, by a blocking copy from pageable memory that has finished when this returns, and only read afterwards, so calls
    on any stream may share it (tests/test_gpu_stream_order.py holds the copy to that)"""
    return _lower(H, W, quality, layout)["params"].to(device)


def encode_jpeg(frames, quality=100, mode="RGB", subsampling="4:2:0"):
    """Frames as baseline JPEG files, the bytes ``PIL.Image.fromarray(f).save(file, 'JPEG', quality=quality, subsampling=subsampling)``
    writes: a ``JpegBatch``.

    frames       mode "RGB": device uint8 (...,H,W,3), what ``export_images``, ``composite_frames`` and ``pyramid_frames`` return; mode "L":
                 device uint8 (...,H,W), what ``export_images(x, "mask")`` returns, written as greyscale files (``Image.fromarray`` of a 2-D
                 array).  Any byte alignment; other strides go through ``.contiguous()``.  Float input is refused: ``export_images`` makes
                 the bytes.
    quality      int in 1..100, libjpeg's scale (the scripts use 100)
    mode         "RGB" or "L"
    subsampling  "4:4:4", "4:2:2" or "4:2:0" (Pillow's default for RGB), or Pillow's ints 0, 1, 2 in that order; it stays at its default
                 with mode "L"

    ``batch[i]`` is file i as bytes, ``batch.write(paths)`` writes them, ``batch.shape`` keeps the leading dimensions (files are in
    row-major order over them).  Two device-to-host copies: the n + 1 offsets, then exactly the bytes used.  ``batch.buffer`` is pinned host
    memory and stays allocated for as long as the batch is held: take ``bytes`` or ``write`` and drop the batch rather than collecting batches.
    The 5 KB table of a (device, H, W, quality, mode, subsampling) is uploaded on the first call and stays resident.  ValueError: another
    dtype or the wrong channel count for the mode, an empty batch, a quality outside 1..100, a frame larger than 65535 or of more than 2^20
    blocks, an unknown mode or subsampling, a subsampling with mode "L".

        batch = encode_jpeg(pyramid_frames(pred, Xa, idx, **preset("tool/generate_market_test", B)))
        batch.write(names)                                                # was: per image to_pil_image(...).save(name, 'JPEG', quality=100)"""
    layout = check_layout(mode, subsampling)
    n, H, W = check_frames(frames, quality, "(...,H,W)" if layout == "L" else "(...,H,W,3)")
    low = _lower(H, W, int(quality), layout)
    N.require_device(frames)
    return _collect(_launch_encode(frames.detach().contiguous(), n, low), n, low, frames.shape[:-2] if layout == "L" else frames.shape[:-3])


def _launch_encode(x, n, low, with_coef=False):
    """``mm_jpeg_modes_encode`` of the dense frames x on the current stream, nothing copied yet: the workspace that holds the results.
    with_coef: the caller goes on to read the coefficients in it, so where they lie is held to ``lower_jpeg`` as well"""
    dev, H, W = x.device, low["H"], low["W"]
    host, par = low["params"], _resident_params(dev, H, W, low["quality"], low["layout"])
    d = N.MMJpegModesDesc()
    d.n, d.H, d.W, d.header_bytes = n, H, W, len(low["header"])
    d.mode, d.sampling = MODES[low["mode"]], SAMPLINGS[low["layout"]]
    d.frames, d.params_host, d.params = N.ptr(x), ctypes.c_void_p(host.data_ptr()), N.ptr(par)
    want = (low["workspace_bytes"](n), low["files_offset"](n)) + ((low["coef_offset"](n),) if with_coef else ())
    ws = N.checked_workspace("mm_jpeg_modes_query_workspace", d, dev, want, ("mm_jpeg_modes_files_offset", "mm_jpeg_modes_coef_offset")[:len(want) - 1],
                             lambda got, want: "mm_jpeg_modes_query_workspace gives %s (bytes, where the files start%s), lower_jpeg %s"
                             % (got, ", where the coefficients do" if with_coef else "", want))
    N.call("mm_jpeg_modes_encode", dev, d)
    return ws


def _collect(ws, n, low, lead):
    """the files out of ``mm_jpeg_modes_encode``'s workspace: a ``JpegBatch`` after two blocking copies, the n + 1 offsets and the bytes used"""
    off, buf = N.read_back(ws, n + 1, low["files_offset"](n))
    return JpegBatch(buf, off, lead)


def check_roundtrip(frames, quality, mode, files, subsampling="4:2:0"):
    """the argument errors of ``jpeg_roundtrip``, before anything touches a device: (n, H, W, layout).  Mode "RGB" has ``encode_jpeg``'s
    (``check_layout``, ``check_frames``); mode "L" the same for (...,H,W)."""
    layout = check_layout(mode, subsampling)
    if mode == "RGB":
        return check_frames(frames, quality) + (layout,)
    if files:
        raise ValueError("files=True needs mode 'RGB': the round trip of a mask forms no file (encode_jpeg(mask, mode='L') writes it)")
    return check_frames(frames, quality, "(...,H,W)") + (layout,)


def jpeg_roundtrip(frames, quality=100, mode="RGB", as_float=False, files=False, subsampling="4:2:0"):
    """Frames as the evaluation reads them back from disk: to the byte, what ``Image.open(file)`` gives for the JPEG file
    ``Image.fromarray(f).save(file, 'JPEG', quality=quality)`` writes of every frame f -- the reference scores these, never the renders
    (trainer.py:697-795, test.py:302-455).  No file is parsed: a file's content is its quantised coefficients, and libjpeg's decoder is
    integer arithmetic from there (dequantise, the islow inverse DCT, "fancy" chroma upsampling, fixed-point YCbCr -> RGB; DESIGN.md and
    csrc/mm_jpeg.hip have the order and the edge rules).

    frames       mode "RGB": device uint8 (...,H,W,3), ``encode_jpeg``'s input with its validation; the result is ``.convert('RGB')`` of the
                 colour file of that subsampling, uint8 (...,H,W,3).  Mode "L": device uint8 (...,H,W), a mask as
                 ``export_images(x, "mask")`` leaves it; the result is the reopened greyscale file (``Image.fromarray(m).save(...)`` of a
                 2-D array; ``.convert('L')`` of it is its samples), uint8 (...,H,W).  That file is not formed here;
                 ``encode_jpeg(m, quality, mode="L")`` writes it.
    subsampling  mode "RGB": ``encode_jpeg``'s, the file that is reopened: 4:2:0 upsamples chroma h2v2, 4:2:2 h2v1 ("fancy" where the
                 chroma plane is wider than two columns, replication otherwise), 4:4:4 not at all.  It stays at its default with mode "L".
    quality      int in 1..100
    as_float     the same values as float32 ``v / 255`` in planes, (...,3,H,W) or (...,H,W): ``to_tensor`` of the reopened image, ready for
                 ``ssim`` / ``recon_scores_as_saved``; the convention of ``export_images(as_float=True)``
    files        mode "RGB" only: return ``(decoded, JpegBatch)`` from ONE transform pass; the batch is
                 ``encode_jpeg(frames, quality, subsampling=subsampling)`` byte for byte and the decoded frames come from the very coefficients those files carry

    The outputs are fresh device tensors, frames is left unmodified, leading dimensions are kept, and nothing synchronises -- unless
    files=True, where ``encode_jpeg``'s two copies happen.  The clamp after the inverse DCT saturates, as libjpeg-turbo's SIMD code does;
    libjpeg's plain C table wraps for samples outside -384..639, which a frame that was itself 8-bit before the forward transform does not
    produce at any quality the tests reach (tests/test_jpeg_roundtrip_host.py counts it).  ValueError: as ``encode_jpeg``, files=True with
    mode "L".

        rgb, mask = export_images(pred, "rgb+mask")                       # was: per image save(name, 'JPEG', quality=100), then
        rec = jpeg_roundtrip(rgb, as_float=True)                          #      to_tensor(Image.open(name).convert('RGB'))
        rec_mask = jpeg_roundtrip(mask, mode="L", as_float=True)          #      to_tensor(Image.open(mask_name).convert('L'))"""
    n, H, W, layout = check_roundtrip(frames, quality, mode, files, subsampling)
    low = _lower(H, W, int(quality), layout)
    N.require_device(frames)
    x = frames.detach().contiguous()
    dev, rgb = x.device, mode == "RGB"
    lead = tuple(frames.shape[:-3] if rgb else frames.shape[:-2])
    shape = lead + (((3, H, W) if as_float else (H, W, 3)) if rgb else (H, W))
    out = torch.empty(shape, dtype=torch.float32 if as_float else torch.uint8, device=dev)
    d = N.MMJpegRoundtripDesc()
    d.n, d.H, d.W, d.mode, d.as_float, d.sampling = n, H, W, MODES[mode], int(bool(as_float)), SAMPLINGS[layout]
    d.frames, d.params_host, d.params, d.out = N.ptr(x), ctypes.c_void_p(low["params"].data_ptr()), N.ptr(_resident_params(dev, H, W, int(quality), layout)), N.ptr(out)
    enc = None
    if files:
        enc = _launch_encode(x, n, low, with_coef=True)
        d.coef = enc.data_ptr() + low["coef_offset"](n)
    ws = N.checked_workspace("mm_jpeg_roundtrip_query_workspace", d, dev, (low["roundtrip_workspace_bytes"](n, mode, own_coef=not files),), (),
                             lambda got, want: "mm_jpeg_roundtrip_query_workspace gives %d bytes, lower_jpeg %d" % (got[0], want[0]))
    N.call("mm_jpeg_roundtrip", dev, d)
    del ws                                                               # (the allocator keeps it for the stream until the kernels are through)
    return (out, _collect(enc, n, low, lead)) if files else out
