"""A token-level deflate emitter and a PNG assembler for the PNG decoder's tests: the counterpart of tests/jpeg_writer.py.

The emitter writes what the TEST chooses -- stored blocks, fixed-code blocks, dynamic blocks with given code lengths and a given
run-length coding of the header, literal / match tokens -- so a test reaches a named corner of RFC 1951 instead of hoping zlib's encoder
goes there.  The assembler puts any stream into a PNG of any colour type and depth, filters rows with a forced type per row (in numpy),
splits IDAT at chosen byte offsets, adds extra chunks, and computes the CRCs over whatever bytes it is given, so damaged streams pass the
parser.  tests/test_png_decode_host.py checks every clean stream it emits with zlib."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length 3..258; 258 is symbol 285"""
    i = max(k for k in range(29) if LENGTH_BASE[k] <= length)
    return 257 + i, LENGTH_EXTRA[i], length - LENGTH_BASE[i]


def distance_symbol(dist):
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


def canonical(lens):
    """symbol -> (code, length) of the canonical Huffman code of ``lens`` (RFC 1951 3.2.2); any lengths, valid or not"""
    count = [0] * 17
    for v in lens:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for L in range(1, 17):
        code = (code + count[L - 1]) << 1
        nxt[L] = code
    out = {}
    for s, v in enumerate(lens):
        if v:
            out[s] = (nxt[v], v)
            nxt[v] += 1
    return out


def complete_lengths(used, n):
    """n code lengths, a complete code over the symbols ``used`` (balanced: lengths m - 1 and m); one symbol gets a partner to be complete"""
    used = sorted(set(used))
    if len(used) == 1:
        used = sorted(set(used + [(used[0] + 1) % n]))
    k = len(used)
    m = max(1, (k - 1).bit_length())
    short = (1 << m) - k
    lens = [0] * n
    for j, s in enumerate(used):
        lens[s] = m - 1 if j < short else m
    return lens


class Deflate:
    """A raw deflate stream written block by block, least significant bit first.  ``marks`` records (bit offset, what) for the tests."""

    def __init__(self):
        self.acc, self.n, self.out, self.marks = 0, 0, bytearray(), []

    def bitpos(self):
        return 8 * len(self.out) + self.n

    def put(self, value, nbits):
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """a Huffman code: its most significant bit first"""
        for k in range(length - 1, -1, -1):
            self.put(code >> k & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc & 255]) if self.n else b"")

    def stored(self, data, final=False, nlen=None):
        self.marks.append((self.bitpos(), "stored"))
        self.put(int(final), 1)
        self.put(0, 2)
        self.align()
        self.put(len(data), 16)
        self.put(~len(data) & 0xFFFF if nlen is None else nlen, 16)
        self.out += bytes(data)
        return self

    def tokens(self, tokens, ll, dd):
        for t in tokens:
            if isinstance(t, int):
                self.code(*ll[t])
            elif t[0] == "m":
                s, eb, ev = length_symbol(t[1])
                if len(t) > 3:                                       # ("m", length, dist, symbol): a chosen symbol (284 + 31 for 258)
                    s, eb, ev = t[3], LENGTH_EXTRA[t[3] - 257], t[1] - LENGTH_BASE[t[3] - 257]
                self.code(*ll[s])
                self.put(ev, eb)
                d, db, dv = distance_symbol(t[2])
                self.code(*dd[d])
                self.put(dv, db)
            elif t[0] == "ll":                                       # a raw literal/length symbol (256, 286, ...)
                self.code(*ll[t[1]])
            elif t[0] == "d":                                        # a raw distance symbol and its extra value
                self.code(*dd[t[1]])
                self.put(t[2], DIST_EXTRA[t[1]] if t[1] < 30 else 0)
            elif t[0] == "bits":
                self.put(t[1], t[2])
            else:
                raise ValueError(t)

    def fixed(self, tokens, final=False, end=True):
        self.marks.append((self.bitpos(), "fixed"))
        self.put(int(final), 1)
        self.put(1, 2)
        self.tokens(list(tokens) + ([("ll", 256)] if end else []), canonical(FIXED_LL), canonical(FIXED_D))
        return self

    def dynamic(self, tokens, ll_lens, d_lens, final=False, end=True, header=None, cl_lens=None, hclen=None, hlit=None, hdist=None):
        """a dynamic block with the given code lengths.  header: the run-length coding of ll_lens + d_lens as items v (a length 0..15),
        (16, n), (17, n) or (18, n); default one item per length.  cl_lens: the 19 lengths of the code-length code; default a complete
        balanced code over the items' symbols.  hclen: how many of them are sent (default up to the last non-zero in transmission order)."""
        self.marks.append((self.bitpos(), "dynamic"))
        ll_lens, d_lens = list(ll_lens), list(d_lens)
        hlit = max(257, len(ll_lens)) if hlit is None else hlit
        hdist = max(1, len(d_lens)) if hdist is None else hdist
        ll_lens += [0] * (hlit - len(ll_lens))
        d_lens += [0] * (hdist - len(d_lens))
        if header is None:
            header = ll_lens + d_lens
        if cl_lens is None:
            cl_lens = complete_lengths([h if isinstance(h, int) else h[0] for h in header], 19)
        if hclen is None:
            hclen = max([4] + [k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]])
        self.put(int(final), 1)
        self.put(2, 2)
        self.put(hlit - 257, 5)
        self.put(hdist - 1, 5)
        self.put(hclen - 4, 4)
        for k in range(hclen):
            self.put(cl_lens[CL_ORDER[k]], 3)
        cl = canonical(cl_lens)
        for h in header:
            if isinstance(h, int):
                self.code(*cl[h])
            else:
                self.code(*cl[h[0]])
                self.put(h[1] - (11 if h[0] == 18 else 3), 7 if h[0] == 18 else 3 if h[0] == 17 else 2)
        self.tokens(list(tokens) + ([("ll", 256)] if end else []), canonical(ll_lens), canonical(d_lens))
        return self


def zlib_wrap(deflate, level_bits=0):
    """the two header bytes (CM 8, CINFO 7), the stream, and the Adler-32 of what zlib inflates it to (0 if it does not inflate)"""
    cmf, flg = 0x78, level_bits << 6
    flg += 31 - (cmf << 8 | flg) % 31
    try:
        d = zlib.decompressobj(-15)
        adler = zlib.adler32(d.decompress(bytes(deflate)))
    except zlib.error:
        adler = 0
    return bytes([cmf, flg]) + bytes(deflate) + struct.pack(">I", adler)


def chunk(kind, body, crc=None):
    body = bytes(body)
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) if crc is None else crc)


def pack_samples(samples, depth):
    """(H, W) samples of 1, 2, 4 or 8 bits as (H, row_bytes) uint8, the high bits first; (H, W, C) 8-bit pixels as (H, W * C)"""
    a = np.asarray(samples)
    if depth == 8:
        return a.reshape(a.shape[0], -1).astype(np.uint8)
    H, W = a.shape
    bits = (a[:, :, None] >> np.arange(depth - 1, -1, -1)) & 1
    return np.packbits(bits.reshape(H, W * depth).astype(np.uint8), axis=1)


def filter_rows(rows, bpp, filters):
    """(H, row_bytes) raw rows as the filtered stream: row y with the forced type filters[y % len(filters)] (a type above 4 is written as it
    is, over the unfiltered bytes)"""
    rows = np.asarray(rows, dtype=np.uint8)
    H, rb = rows.shape
    out = np.zeros((H, 1 + rb), dtype=np.uint8)
    z = np.zeros(rb, dtype=np.int32)
    for y in range(H):
        ft = filters[y % len(filters)]
        cur, up = rows[y].astype(np.int32), (rows[y - 1].astype(np.int32) if y else z)
        left = np.concatenate([z[:bpp], cur[:-bpp]])[:rb] if rb > bpp else z
        ul = np.concatenate([z[:bpp], up[:-bpp]])[:rb] if rb > bpp else z
        if ft == 1:
            pred = left
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (left + up) >> 1
        elif ft == 4:
            p = left + up - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        else:
            pred = z
        out[y, 0] = ft
        out[y, 1:] = (cur - pred) & 255
    return out.tobytes()


def png(W, H, depth, ctype, idat, splits=(), plte=None, trns=None, extra=(), after=(), interlace=0, iend=True):
    """a PNG file around the IDAT data ``idat`` (a whole zlib stream), cut into IDAT chunks at the byte offsets ``splits``; extra: chunks
    (kind, body) before IDAT, after: behind it"""
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, interlace))]
    if plte is not None:
        out.append(chunk(b"PLTE", plte))
    if trns is not None:
        out.append(chunk(b"tRNS", trns))
    out += [chunk(k, b) for k, b in extra]
    cuts = [0] + sorted(splits) + [len(idat)]
    out += [chunk(b"IDAT", idat[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    out += [chunk(k, b) for k, b in after]
    if iend:
        out.append(chunk(b"IEND", b""))
    return b"".join(out)


def png_of(samples, depth, ctype, filters=(0,), deflate=None, **kw):
    """a PNG of ``samples`` ((H, W) or (H, W, C)) with forced row filters; deflate: a function from the filtered stream to a raw deflate
    stream (default zlib level 6)"""
    a = np.asarray(samples)
    H, W = a.shape[:2]
    channels = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    stream = filter_rows(pack_samples(a, depth), 1 if depth < 8 else channels, filters)
    if deflate is None:
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        raw = c.compress(stream) + c.flush()
    else:
        raw = deflate(stream)
    return png(W, H, depth, ctype, zlib_wrap(raw), **kw)
