"""PNG files as device frames, Pillow's pixels: host side of ``mm_png_decode`` (csrc/mm_png_decode.hip, csrc/mm_inflate.h).

Every sample the reference trains on is two files: the photo, a JPEG (``decode_jpeg``), and the mask, a PNG -- ``seg_loader`` is
``Image.open(f).convert('L')`` in datasets/bird.py, atr.py and market.py, ``.convert('RGBA')`` and its alpha plane in datasets/thuman2.py.
``decode_png`` takes the files' bytes and leaves the frames in device memory, packed like ``ImagePool``: one upload (the tables and the
concatenated IDAT data), one memset and three launches whatever the number of files.  Every pixel equals Pillow 12's
``Image.open(f).convert(mode)``: integers on both sides, compared without a tolerance.  It also reads this project's own ``encode_png``
files back.

    frames = decode_png([open(p, "rb").read() for p in paths], "L")    # or the paths themselves, or an encode_png PngBatch
    frames.frames[i]                                                   # (H_i, W_i) uint8 view ((H_i, W_i, 3 or 4) in mode "RGB" / "RGBA")
    pool = ImagePool.from_files(jpegs, pngs, device, mask="market")    # input_batches.py: both decoded straight into the pool's buffer

Accepted: colour types 0 (grey; 1, 2, 4, 8 bits), 2 (RGB, 8), 3 (palette; 1, 2, 4, 8), 4 (grey + alpha, 8), 6 (RGBA, 8); any split of
the IDAT data; tRNS on a palette file; stored, fixed and dynamic deflate blocks; filters 0-4; ancillary chunks skipped; data after the
final block and a missing IEND tolerated.  Files of mixed sizes, types and depths in one call.
Rejected by the parser (ValueError naming the file's index; nothing is launched): no signature, no IHDR, no IDAT, IDAT chunks that are
not consecutive, a bad CRC of a chunk that is read (IHDR, PLTE, tRNS, IDAT, IEND), a chunk length that runs past the file, 16-bit depth,
Adam7 interlace, a depth the colour type does not allow, a missing PLTE for colour type 3, a bad zlib header (CM = 8, CINFO <= 7, FCHECK,
no FDICT), W or H of 0 or above 65535, tRNS on colour types 0 or 2 when mode is "RGBA" (in the other modes Pillow ignores it, and so do
we).  The Adler-32 trailer is NOT verified: the IDAT chunks' CRCs cover the same bytes.
Damaged deflate data is not an error of the parser: the kernel cannot spin, read or write out of range for any bytes, a damaged stream
stops at the damage with the rest of its bytes zero, the unfilter and pixel passes still run, and the file's ``status`` gets ST_* bits.
Such a file's pixels are defined by ``decode_png_host``, not by Pillow (which raises).

Conversions (Pillow's): grey samples of 1 / 2 / 4 bits scale by 255 / 85 / 17; palette indices go through PLTE (an index beyond it is
black); to "L", (19595 R + 38470 G + 7471 B + 32768) >> 16 of palette entries (in the host-built table) and of RGB / RGBA pixels (on the
device), the grey sample of grey and grey + alpha; to "RGB", grey replicated, alpha dropped, tRNS ignored; to "RGBA", alpha 255 where the
file has none, the file's alpha for types 4 and 6, for type 3 the tRNS byte of the index and 255 beyond its length.

Out of scope: 16-bit samples, interlacing, APNG, gamma / ICC / sRGB chunks, verifying Adler-32, splitting one stream over several waves,
reading directories, anything differentiable."""
import os
import zlib

import numpy as np
import torch

from . import _native as N
from .jpeg_decode import DecodedFrames
from .png import MODES

ST_OVERRUN, ST_BAD_BLOCK, ST_BAD_TABLE, ST_BAD_CODE, ST_BAD_DISTANCE, ST_SHORT, ST_BAD_FILTER = 1, 2, 4, 8, 16, 32, 64      # MM_PNG_ST_*
STATUS_NAMES = ((ST_OVERRUN, "OVERRUN"), (ST_BAD_BLOCK, "BAD_BLOCK"), (ST_BAD_TABLE, "BAD_TABLE"), (ST_BAD_CODE, "BAD_CODE"),
                (ST_BAD_DISTANCE, "BAD_DISTANCE"), (ST_SHORT, "SHORT"), (ST_BAD_FILTER, "BAD_FILTER"))
FILE_INTS = N.PNG_DEC_FILE_INTS
(F_H, F_W, F_CTYPE, F_DEPTH, F_BPP, F_ROWB, F_TABLE, F_BEGIN, F_END, F_SOFF) = range(10)
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS_IN = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
LOOK_BITS, MAX_SYMS = 9, 320                                         # MM_INF_LOOK_BITS, MM_INF_MAX_SYMS
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _fail(i, why):
    raise ValueError("file %d: %s" % (i, why))


def parse_png(data, i=0, mode="L"):
    """The chunks of one file (host arithmetic): a dict of H, W, ctype, depth, plte and trns (bytes or None) and idat, the concatenated IDAT
    data.  ValueError for what is rejected, naming file ``i``."""
    n = len(data)
    if n < 8 or bytes(data[:8]) != SIGNATURE:
        _fail(i, "no PNG signature")
    pos, ihdr, plte, trns, idat, closed, first = 8, None, None, None, None, False, True
    while pos < n:
        if pos + 12 > n:
            _fail(i, "the chunk at byte %d runs past the file" % pos)
        length, kind = int.from_bytes(data[pos:pos + 4], "big"), bytes(data[pos + 4:pos + 8])
        if pos + 12 + length > n:
            _fail(i, "the length of chunk %r at byte %d runs past the file" % (kind, pos))
        if first and kind != b"IHDR":
            _fail(i, "no IHDR chunk at the start")
        first = False
        body = data[pos + 8:pos + 8 + length]
        if kind in (b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND") and zlib.crc32(data[pos + 4:pos + 8 + length]) != int.from_bytes(data[pos + 8 + length:pos + 12 + length], "big"):
            _fail(i, "a bad CRC of chunk %r at byte %d" % (kind, pos))
        pos += 12 + length
        if kind == b"IDAT":
            if closed:
                _fail(i, "IDAT chunks that are not consecutive")
            idat = [body] if idat is None else idat + [body]
            continue
        if idat is not None:
            closed = True
        if kind == b"IHDR":
            if ihdr is not None or length != 13:
                _fail(i, "a malformed IHDR chunk")
            ihdr = bytes(body)
        elif kind == b"PLTE":
            if length % 3 or length > 768 or length == 0:
                _fail(i, "a malformed PLTE chunk")
            plte = bytes(body)
        elif kind == b"tRNS":
            trns = bytes(body)
        elif kind == b"IEND":
            break
    if ihdr is None:
        _fail(i, "no IHDR chunk")
    W, H = int.from_bytes(ihdr[0:4], "big"), int.from_bytes(ihdr[4:8], "big")
    depth, ctype, comp, filt, lace = ihdr[8:13]
    if W == 0 or H == 0:
        _fail(i, "a width or height of 0")
    if W > 65535 or H > 65535:
        _fail(i, "%d x %d, more than 65535 pixels a side" % (H, W))
    if ctype not in DEPTHS:
        _fail(i, "colour type %d" % ctype)
    if depth not in DEPTHS[ctype]:
        _fail(i, "a bit depth of %d, which colour type %d does not allow" % (depth, ctype))
    if depth == 16:
        _fail(i, "16-bit samples, only 1 to 8 bits are decoded")
    if comp != 0 or filt != 0:
        _fail(i, "compression method %d / filter method %d" % (comp, filt))
    if lace == 1:
        _fail(i, "Adam7 interlace, only non-interlaced files are decoded")
    if lace != 0:
        _fail(i, "interlace method %d" % lace)
    if idat is None:
        _fail(i, "no IDAT chunk")
    if ctype == 3 and plte is None:
        _fail(i, "colour type 3 without a PLTE chunk")
    if trns is not None and ctype in (0, 2) and mode == "RGBA":
        _fail(i, "a tRNS chunk on colour type %d with mode 'RGBA' (a colour key is not part of this)" % ctype)
    idat = b"".join(bytes(b) for b in idat)
    if len(idat) < 2 or (idat[0] & 15) != 8 or (idat[0] >> 4) > 7 or (idat[0] << 8 | idat[1]) % 31 or (idat[1] & 32):
        _fail(i, "a bad zlib header (CM = 8, CINFO <= 7, FCHECK, no FDICT)")
    return dict(H=H, W=W, ctype=ctype, depth=depth, plte=plte, trns=trns if ctype == 3 else None, idat=idat)


def luma(r, g, b):
    """Pillow's L of RGB"""
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16


def conversion_table(ctype, depth, plte, trns, mode):
    """the 256 words of a grey (type 0) or palette (type 3) file for output ``mode``: for sample / index v the output pixel, channel c in
    byte c (mode "L": byte 0)"""
    t = np.zeros(256, dtype=np.uint32)
    for v in range(1 << depth):
        if ctype == 0:
            r = g = b = v * (255 // ((1 << depth) - 1))
            a = 255
        else:
            r, g, b = plte[3 * v:3 * v + 3] if 3 * v + 3 <= len(plte) else (0, 0, 0)
            a = trns[v] if trns is not None and v < len(trns) else 255
        t[v] = luma(r, g, b) if mode == "L" else r | g << 8 | b << 16 | (a << 24 if mode == "RGBA" else 0)
    return t


def _read(f, i):
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    if isinstance(f, (str, os.PathLike)):
        with open(f, "rb") as h:
            return h.read()
    raise ValueError("file %d: need bytes, a bytearray or a path, got %s" % (i, type(f)))


def lower_png_decode(files, mode="L"):
    """Files as the tables ``mm_png_decode`` reads (host arithmetic only, no device; MMPngDecodeDesc in include/mm_render.h has the
    layouts): a dict of n; mode; channels; data, the files' raw deflate streams back to back (uint8: each file's IDAT payloads concatenated,
    without the two zlib header bytes); files (n, 16) int32, the per-file records; offsets (n + 1) int64 and sizes (n, 2) int32 rows (H, W),
    the packing of the output; conv (T, 256) uint32, the conversion tables of the grey and palette files, deduplicated over the batch;
    tables, all of these as the one int32 array the library takes; stream_bytes, status_offset and workspace_bytes
    (mm_png_decode_query_workspace in Python).  Every chunk that is read has its CRC checked (zlib.crc32) and the zlib header is checked
    here; the Adler-32 trailer is not verified (the CRCs cover the same bytes).  ValueError, naming the file's index and the reason, for
    everything the parser rejects."""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError("mode must be 'L', 'RGB' or 'RGBA', got %r" % (mode,))
    blobs = [_read(f, i) for i, f in enumerate(files)]
    if not blobs:
        raise ValueError("an empty list of files")
    n = len(blobs)
    if n > N.PNG_DEC_MAX_FILES:
        raise ValueError("%d files: at most %d in a call" % (n, N.PNG_DEC_MAX_FILES))
    recs = np.zeros((n, FILE_INTS), dtype=np.int32)
    cindex, streams = {}, []
    at = soff = 0
    for i, blob in enumerate(blobs):
        h = parse_png(blob, i, mode)
        ctype, depth = h["ctype"], h["depth"]
        cin = CHANNELS_IN[ctype]
        rowb = (h["W"] * cin * depth + 7) // 8
        table = -1
        if ctype in (0, 3):
            key = (ctype, depth, h["plte"] if ctype == 3 else None, h["trns"] if mode == "RGBA" else None)
            if key not in cindex:
                cindex[key] = (len(cindex), conversion_table(ctype, depth, h["plte"], key[3], mode))
            table = cindex[key][0]
        stream = h["idat"][2:]
        recs[i, :F_SOFF + 1] = (h["H"], h["W"], ctype, depth, 1 if depth < 8 else cin, rowb, table, at, at + len(stream), soff)
        streams.append(stream)
        at, soff = at + len(stream), soff + h["H"] * (1 + rowb)
        if at > N.PNG_DEC_MAX_BYTES or soff > N.PNG_DEC_MAX_BYTES:
            raise ValueError("files 0..%d have %d bytes of deflate data and %d of inflated rows, more than %d in a call" % (i, at, soff, N.PNG_DEC_MAX_BYTES))
    sizes = recs[:, :2].copy()
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(sizes[:, 0].astype(np.int64) * sizes[:, 1], out=offsets[1:])
    if offsets[-1] > N.PNG_DEC_MAX_PIXELS:
        raise ValueError("%d pixels, more than %d in a call" % (offsets[-1], N.PNG_DEC_MAX_PIXELS))
    data = np.frombuffer(b"".join(streams) or b"\0", dtype=np.uint8)      # (a file's stream may be empty; the call's bytes may not)
    conv = np.stack([c for _, c in sorted(cindex.values(), key=lambda e: e[0])]) if cindex else np.zeros((0, 256), dtype=np.uint32)
    tables = np.concatenate([recs.reshape(-1), offsets.view(np.int32), conv.view(np.int32).reshape(-1)])
    status_offset = N.up256(soff)
    return dict(n=n, mode=mode, channels=MODES[mode][0], data=data, files=recs, offsets=offsets, sizes=sizes, conv=conv, tables=tables,
                stream_bytes=soff, status_offset=status_offset, workspace_bytes=status_offset + N.up256(4 * n))


# ---- the decoder restated on the host, in the kernels' order ------------------------------------------------------------------------------
def _rev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2)


_REV15 = [_rev(x, 15) for x in range(1 << 15)]


def build_table(lens):
    """``inf_build`` of csrc/mm_inflate.h: (look, maxcode, valoff, syms, max length, over-subscribed, incomplete) of the code lengths"""
    count = [0] * 16
    for v in lens:
        count[v] += 1
    maxcode, valoff, off = [-1] * 16, [0] * 16, [0] * 16
    code = k = mx = 0
    left = 1
    for L in range(1, 16):
        c = count[L]
        left = 2 * left - c
        if left < 0:
            return None, None, None, None, mx, True, False
        if c:
            mx = L
        off[L], valoff[L], maxcode[L] = k, k - code, (code + c - 1 if c else -1)
        code, k = (code + c) << 1, k + c
    syms = [0] * MAX_SYMS
    fill = list(off)
    for s, v in enumerate(lens):
        if v:
            syms[fill[v]] = s
            fill[v] += 1
    look = [0] * (1 << LOOK_BITS)
    for e in range(1 << LOOK_BITS):
        rev = _rev(e, LOOK_BITS)
        for L in range(1, LOOK_BITS + 1):
            c = rev >> (LOOK_BITS - L)
            if c <= maxcode[L]:
                idx = c + valoff[L]
                if 0 <= idx < MAX_SYMS:
                    look[e] = L << 12 | syms[idx]
                break
    return look, maxcode, valoff, syms, mx, False, left > 0


_FIXED = None


def fixed_tables():
    global _FIXED
    if _FIXED is None:
        _FIXED = (build_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), build_table([5] * 32))
    return _FIXED


class HostInflate:
    """``inflate_stream`` of csrc/mm_inflate.h in Python: raw[begin:end] into out[base:base + S] (a zeroed uint8 array); ``run`` returns
    the status.  counters: a dict that receives what the stream reached (the tests assert through it); pitch: bytes of a filtered row, for
    the ("rowcross",) counter only.  The small methods are what the tests' fault copies override."""

    def __init__(self, raw, begin, end, out, base, S, counters=None, pitch=0):
        self.raw, self.begin, self.end, self.out, self.base, self.S = raw, begin, end, out, base, S
        self.o = self.acc = self.n = 0
        self.pos = begin
        self.c = counters
        self.pitch = pitch

    def note(self, *key):
        if self.c is not None:
            self.c[key] = self.c.get(key, 0) + 1

    def byte(self, at):
        return self.raw[at] if self.begin <= at < self.end else 0

    def fill(self):
        if self.n <= 32:
            w = self.byte(self.pos) | self.byte(self.pos + 1) << 8 | self.byte(self.pos + 2) << 16 | self.byte(self.pos + 3) << 24
            self.acc |= w << self.n
            self.pos += 4
            self.n += 32

    def bits(self, k):
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def consumed(self):
        return 8 * (self.pos - self.begin) - self.n

    def overrun(self):
        return self.consumed() > 8 * (self.end - self.begin)

    def symbol(self, t):
        look, maxcode, valoff, syms = t[:4]
        peek = self.acc & 0x7FFF
        e = look[peek & ((1 << LOOK_BITS) - 1)]
        if e:
            self.bits(e >> 12)
            return e & 0xFFF
        rev = _REV15[peek]
        for L in range(LOOK_BITS + 1, 16):
            c = rev >> (15 - L)
            if c <= maxcode[L]:
                idx = c + valoff[L]
                if not 0 <= idx < MAX_SYMS:
                    return -1
                self.bits(L)
                return syms[idx]
        return -1

    def copy_match(self, length, dist):
        """min(dist, 64) bytes a step, every byte of a step older than the step"""
        todo = min(length, self.S - self.o)
        step = min(dist, 64)
        while todo > 0:
            k = min(todo, step)
            at = self.base + self.o
            self.out[at:at + k] = self.out[at - dist:at - dist + k].copy()
            self.o += k
            todo -= k

    def read_lengths(self, total, hlit, cl):
        """the hlit + hdist code lengths of a dynamic header, through the code-length code ``cl``: (lens, status)"""
        lens, prev = [], 0
        while len(lens) < total:
            self.fill()
            sym = self.symbol(cl)
            if sym < 0:
                return lens, ST_BAD_TABLE
            rep, v = 1, sym
            if sym == 16:
                v, rep = prev, 3 + self.bits(2)
            elif sym == 17:
                v, rep = 0, 3 + self.bits(3)
            elif sym == 18:
                v, rep = 0, 11 + self.bits(7)
            if self.overrun():
                return lens, ST_OVERRUN
            if (sym == 16 and not lens) or len(lens) + rep > total:
                return lens, ST_BAD_TABLE
            if sym >= 16:
                self.note("rep", sym)
                if len(lens) < hlit < len(lens) + rep:
                    self.note("rep_cross")
            lens += [v] * rep
            prev = v
        return lens, 0

    def dynamic_header(self):
        self.fill()
        hlit, hdist, hclen = self.bits(5) + 257, self.bits(5) + 1, self.bits(4) + 4
        if self.overrun():
            return None, None, ST_OVERRUN
        if hlit > 286 or hdist > 30:
            return None, None, ST_BAD_TABLE
        cll = [0] * 19
        for i in range(hclen):
            self.fill()
            cll[CL_ORDER[i]] = self.bits(3)
        if self.overrun():
            return None, None, ST_OVERRUN
        cl = build_table(cll)
        if cl[5] or cl[6]:
            return None, None, ST_BAD_TABLE
        lens, st = self.read_lengths(hlit + hdist, hlit, cl)
        if st:
            return None, None, st
        if lens[256] == 0:
            return None, None, ST_BAD_TABLE
        ll = build_table(lens[:hlit])
        if ll[5] or (ll[6] and ll[4] != 1):
            return None, None, ST_BAD_TABLE
        dd = build_table(lens[hlit:])
        if dd[5] or (dd[6] and dd[4] > 1):
            return None, None, ST_BAD_TABLE
        self.note("codelen", max(ll[4], dd[4]))
        self.note("dcodes", sum(1 for v in lens[hlit:] if v))
        return ll, dd, 0

    def read_match(self, sym, dd):
        """a length symbol's extra bits, the distance symbol and its extra bits: (length, distance, status)"""
        i = sym - 257
        le = 0 if i < 8 or i == 28 else (i >> 2) - 1
        length = (258 if i == 28 else 3 + i if i < 8 else 3 + ((4 + (i & 3)) << le)) + self.bits(le)
        self.fill()
        d = self.symbol(dd)
        if d < 0 or d > 29:
            return 0, 0, ST_BAD_CODE
        de = 0 if d < 4 else (d >> 1) - 1
        dist = (1 + d if d < 4 else 1 + ((2 + (d & 1)) << de)) + self.bits(de)
        self.note("lsym", sym)
        self.note("dsym", d)
        return length, dist, 0

    def block(self, ll, dd):
        while True:
            self.fill()
            sym = self.symbol(ll)
            if sym < 0:
                return ST_BAD_CODE
            if sym < 256:
                if self.overrun():
                    return ST_OVERRUN
                self.out[self.base + self.o] = sym
                self.o += 1
                if self.o == self.S:
                    return 0
                continue
            if sym == 256:
                return ST_OVERRUN if self.overrun() else 0
            if sym > 285:
                return ST_BAD_CODE
            length, dist, st = self.read_match(sym, dd)
            if st:
                return st
            if self.overrun():
                return ST_OVERRUN
            if dist > self.o:
                return ST_BAD_DISTANCE
            self.note("dist", dist)
            if dist < length:
                self.note("overlap")
            if self.pitch and self.o // self.pitch != (min(self.o + length, self.S) - 1) // self.pitch:
                self.note("rowcross")
            self.copy_match(length, dist)
            if self.o == self.S:
                return 0

    def run(self):
        if self.S <= 0:
            return 0
        while True:
            self.note("align", self.consumed() % 8)
            self.fill()
            last, kind = self.bits(1), self.bits(2)
            if self.overrun():
                return ST_OVERRUN
            if kind == 3:
                return ST_BAD_BLOCK
            self.note("block", kind)
            if kind == 0:
                self.bits(self.n & 7)
                self.fill()
                length, nlen = self.bits(16), self.bits(16)
                if self.overrun():
                    return ST_OVERRUN
                if length ^ nlen != 0xFFFF:
                    return ST_BAD_BLOCK
                self.note("stored", length)
                p = self.pos - (self.n >> 3)
                want = min(length, self.S - self.o)
                have = max(self.end - p, 0)
                k = min(want, have)
                at = self.base + self.o
                self.out[at:at + k] = np.frombuffer(self.raw[p:p + k], dtype=np.uint8)
                self.o += k
                if want > have:
                    return ST_OVERRUN
                self.pos, self.n, self.acc = p + length, 0, 0
            else:
                if kind == 1:
                    ll, dd = fixed_tables()
                else:
                    ll, dd, st = self.dynamic_header()
                    if st:
                        return st
                st = self.block(ll, dd)
                if st:
                    return st
            if self.o == self.S:
                if self.consumed() < 8 * (self.end - self.begin) - 32:
                    self.note("trailing")
                return 0
            if last:
                return ST_SHORT


class HostPixels:
    """The unfilter and pixel passes in numpy / Python, the kernels' arithmetic; the small methods are what the tests' fault copies override."""

    def __init__(self, counters=None):
        self.c = counters

    def note(self, *key):
        if self.c is not None:
            self.c[key] = self.c.get(key, 0) + 1

    def average(self, a, b):
        return (a + b) >> 1                                          # (a 9-bit sum)

    def paeth(self, a, b, c):
        pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
        if pa == pb and pa <= pc:
            self.note("paeth_tie", "ab")
        if pa == pc and pa <= pb:
            self.note("paeth_tie", "ac")
        if pb == pc and pb < pa:
            self.note("paeth_tie", "bc")
        return a if pa <= pb and pa <= pc else b if pb <= pc else c

    def unfilter(self, S, H, rowb, bpp):
        """the stream S (H rows of 1 + rowb bytes, a uint8 array) unfiltered in place: the status (0 or ST_BAD_FILTER)"""
        rows = S.reshape(H, 1 + rowb)
        st = 0
        prev = [0] * rowb
        for y in range(H):
            ft = int(rows[y, 0])
            if ft > 4:
                st, ft = ST_BAD_FILTER, 0
            self.note("filter", ft, y == 0, bpp)
            cur = rows[y, 1:].tolist()
            if ft == 1:
                for x in range(bpp, rowb):
                    cur[x] = (cur[x] + cur[x - bpp]) & 255
            elif ft == 2:
                cur = [(v + u) & 255 for v, u in zip(cur, prev)]
            elif ft == 3:
                for x in range(rowb):
                    cur[x] = (cur[x] + self.average(cur[x - bpp] if x >= bpp else 0, prev[x])) & 255
            elif ft == 4:
                for x in range(rowb):
                    cur[x] = (cur[x] + (self.paeth(cur[x - bpp], prev[x], prev[x - bpp]) if x >= bpp else self.paeth(0, prev[x], 0))) & 255
            rows[y, 1:] = cur
            prev = cur
        return st

    def unpack(self, rows, depth, W):
        """(H, rowb) packed rows as (H, W) samples: the high bits first"""
        bits = np.unpackbits(rows, axis=1)[:, :W * depth].reshape(rows.shape[0], W, depth)
        return (bits.astype(np.uint32) << np.arange(depth - 1, -1, -1, dtype=np.uint32)).sum(axis=2).astype(np.uint32)

    def pixels(self, S, rec, conv, mode):
        H, W, ctype, depth, _, rowb, table = (int(v) for v in rec[:7])
        rows = np.ascontiguousarray(S.reshape(H, 1 + rowb)[:, 1:])
        if ctype in (0, 3):
            e = conv[table][self.unpack(rows, depth, W) if depth < 8 else rows.astype(np.uint32)]
        else:
            px = rows.reshape(H, W, CHANNELS_IN[ctype]).astype(np.uint32)
            if ctype == 4:
                e = px[..., 0] if mode == "L" else px[..., 0] * 0x010101 | px[..., 1] << 24
            else:
                r, g, b = px[..., 0], px[..., 1], px[..., 2]
                a = px[..., 3] if ctype == 6 else np.uint32(255)
                e = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16 if mode == "L" else r | g << 8 | b << 16 | a << 24
        e = e.astype(np.uint32)
        if mode == "L":
            return (e & 255).astype(np.uint8)
        return np.stack([(e >> (8 * c)) & 255 for c in range(MODES[mode][0])], axis=2).astype(np.uint8)


def decode_png_host(files, mode="L", counters=None, inflate=HostInflate, pixels=HostPixels):
    """The whole decoder on the host, in numpy / Python, in the kernels' order: (frames, status) -- a list of (H_i, W_i) uint8 arrays
    ((H_i, W_i, 3) / (H_i, W_i, 4) in modes "RGB" / "RGBA") and the (n) int32 status words.  The yardstick where Pillow is not installed, and
    the definition of what a damaged file decodes to; tests/test_png_decode_host.py holds it to Pillow and to zlib.  Every index it forms
    stays inside the file's bytes and its S bytes (Python raises otherwise; the tests rely on that).  counters: a dict that receives what
    the streams reached; inflate / pixels: the classes to run (the tests' fault copies)."""
    low = files if isinstance(files, dict) else lower_png_decode(files, mode)
    raw = low["data"].tobytes()
    streams = np.zeros(low["stream_bytes"], dtype=np.uint8)
    status = np.zeros(low["n"], dtype=np.int32)
    px = pixels(counters)
    frames = []
    for i, rec in enumerate(low["files"].tolist()):
        H, rowb, soff = rec[F_H], rec[F_ROWB], rec[F_SOFF]
        S = H * (1 + rowb)
        status[i] = inflate(raw, rec[F_BEGIN], rec[F_END], streams, soff, S, counters, 1 + rowb).run()
        status[i] |= px.unfilter(streams[soff:soff + S], H, rowb, rec[F_BPP])
        frames.append(px.pixels(streams[soff:soff + S], rec, low["conv"], low["mode"]))
    return frames, status


# ---- the device path ----------------------------------------------------------------------------------------------------------------------
def status_text(st):
    return "|".join(name for bit, name in STATUS_NAMES if st & bit) or "0"


def _upload(low, device):
    """one pinned host buffer -- the tables, then on a 16-byte boundary the streams' bytes -- and its one copy to the device: (host, dev,
    where the bytes start)"""
    b0 = (4 * low["tables"].size + 15) // 16 * 16
    host = torch.empty(b0 + low["data"].size, dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    hv[:4 * low["tables"].size] = low["tables"].view(np.uint8)
    hv[b0:] = low["data"]
    return host, host.to(device, non_blocking=True), b0


def _launch(low, host, dev_buf, b0, out, workspace=None, post=0):
    """``mm_png_decode`` of an uploaded batch into ``out`` on the current stream: the workspace (its status words at status_offset).
    workspace: a uint8 device tensor to use (at least workspace_bytes, 16-byte aligned) instead of a fresh one; post: MM_PNG_POST_* bits."""
    d = N.MMPngDecodeDesc()
    d.n, d.channels, d.n_tables, d.post, d.n_bytes = low["n"], low["channels"], low["conv"].shape[0], post, low["data"].size
    d.bytes, d.tables_host, d.tables, d.out = dev_buf.data_ptr() + b0, host.data_ptr(), dev_buf.data_ptr(), N.ptr(out)
    if workspace is None:
        ws = N.checked_workspace("mm_png_decode_query_workspace", d, out.device, (low["workspace_bytes"],), (),
                                 lambda got, want: "mm_png_decode_query_workspace gives %d bytes, lower_png_decode %d" % (got[0], want[0]))
    else:
        ws = workspace
        d.workspace, d.workspace_bytes = ws.data_ptr(), low["workspace_bytes"]
    N.call("mm_png_decode", out.device, d)
    return ws


def _decode_into(low, out, strict, workspace=None, post=0):
    """upload, launch, and the status (n) int32 on the device"""
    host, dev_buf, b0 = _upload(low, out.device)
    ws = _launch(low, host, dev_buf, b0, out, workspace, post)
    status = ws[low["status_offset"]:low["status_offset"] + 4 * low["n"]].view(torch.int32)
    if strict:
        bad = [(i, s) for i, s in enumerate(status.tolist()) if s]
        if bad:
            raise ValueError("damaged data in %d of %d files: %s" % (len(bad), low["n"], ", ".join("file %d: %s" % (i, status_text(s)) for i, s in bad)))
    return status


def decode_png(files, mode="L", device=None, out=None, strict=True):
    """PNG files as device frames, Pillow's pixels: a ``DecodedFrames``.

    files    a list of ``bytes`` / ``bytearray`` / paths, or a ``PngBatch`` (``encode_png``'s result); mixed sizes, colour types and bit
             depths in one call
    mode     "L", "RGB" or "RGBA": what ``Image.open(f).convert(mode)`` gives, (H,W), (H,W,3) or (H,W,4)
    device   where to decode (default: ``out``'s device, else the current device)
    out      a dense uint8 device tensor of exactly the bytes needed (1, 3 or 4 per pixel of all files), decoded in place; it may start at
             any byte.  Default: a fresh buffer.
    strict   True: wait for the status and raise ValueError listing the damaged files (the frames are decoded all the same, into ``out``
             if given).  False: nothing waits; ``status`` says which files are damaged, and their pixels are ``decode_png_host``'s.

    One upload (tables and deflate data in one buffer), one memset and three launches, independent of the number of files; no per-file
    host work after parsing.  ValueError for what the parser rejects (see the module's docstring), naming the file's index: nothing is
    launched for a rejected batch.  The Adler-32 trailer is not verified."""
    low = files if isinstance(files, dict) else lower_png_decode(files, mode)
    nbytes = int(low["offsets"][-1]) * low["channels"]
    if out is None:
        dev = torch.device("cuda" if device is None else device)
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != nbytes:
            raise ValueError("out must be a dense uint8 tensor of exactly %d bytes, got %s" % (nbytes, "%s %s" % (out.dtype, tuple(out.shape)) if torch.is_tensor(out) else type(out)))
        if device is not None and torch.device(device).type != out.device.type:
            raise ValueError("out is on %s, device says %s" % (out.device, device))
    N.require_device(out)
    flat = out.view(-1)
    status = _decode_into(low, flat, strict)
    return DecodedFrames(flat, low["offsets"], low["sizes"], status, low["mode"])
