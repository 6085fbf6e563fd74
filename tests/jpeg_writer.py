"""A baseline JPEG writer with everything exposed, for the files no common encoder writes (tests/golden/make_golden_jpeg_foreign.py builds
the fixture with it; tests/test_jpeg_foreign_host.py and tests/test_gpu_jpeg_foreign.py assert on its census).  numpy only, and nothing of the
package: it feeds the decoder under test.

A file is a dict (``model``): H, W; comps, per component (id, h, v, quantisation id); qt, id -> 64 ints in natural order; ht, (class, id) ->
(16 counts, symbols); sel, per component its (DC id, AC id); restart, MCUs per interval (0: none); scan, the entropy-coded bytes with their
RSTn markers, without EOI.

    from_image(img, layout, qt, ht, sel, restart)       samples -> float64 DCT -> quantised blocks -> scan
    from_coefficients(blocks, H, W, layout, ...)        (blocks, 64) int16 in zigzag order, MCU by MCU; refused outside libjpeg's defined range
    parse(file)                                         an existing file as a model: its scan bytes stay untouched
    serialize(model, layout, fill_rst, fill_eoi)        the header's layout is data: a list of segment items (``default_layout``)
    census(file)                                        what the entropy-coded data of a file holds, from its bytes and its own tables

The yardstick of every file is Pillow's decode of it, never the source image: how ``from_image`` downsamples or rounds does not matter."""
import re

import numpy as np

ZIGZAG = sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) % 2 else i % 8))     # natural index of zigzag position k
MCU = {"4:2:0": (6, 2, 2), "4:2:2": (4, 2, 1), "4:4:4": (3, 1, 1), "L": (1, 1, 1)}                        # blocks per MCU, luma h, luma v
AC_SYMBOLS = bytes([0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 11)])                   # every symbol a baseline AC table may hold
DC_SYMBOLS = bytes(range(12))
_C = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])
_RST = re.compile(b"\xff+[\xd0-\xd7]", re.DOTALL)


# ---- Huffman tables as (counts, symbols) ------------------------------------------------------------------------------------------------
def table(symbols, lengths):
    """(16 counts, symbols) with symbols[i] on a code of lengths[i] bits (a list, or one length for all); ValueError if the lengths
    oversubscribe the code space or would use an all-ones code"""
    symbols = bytes(symbols)
    if isinstance(lengths, int):
        lengths = [lengths] * len(symbols)
    order = sorted(range(len(symbols)), key=lambda i: lengths[i])                 # stable: the given order inside a length
    counts = [sum(1 for v in lengths if v == n) for n in range(1, 17)]
    if len(lengths) != len(symbols) or sum(counts) != len(symbols) or sum(c << (16 - n) for n, c in enumerate(counts, 1)) >= 1 << 16:
        raise ValueError("code lengths %s do not fit a prefix code without the all-ones code" % (counts,))
    return bytes(counts), bytes(symbols[i] for i in order)


def flat_table(symbols):
    """all symbols at the shortest common length"""
    return table(symbols, len(symbols).bit_length())


def ladder_table(symbols):
    """one code each of lengths 1 to 8 (the first eight symbols), the rest at 16"""
    return table(symbols, list(range(1, 9)) + [16] * (len(symbols) - 8))


def split_table(symbols, short, long):
    """the first half of the symbols at ``short`` bits, the second at ``long``"""
    half = len(symbols) // 2
    return table(symbols, [short] * half + [long] * (len(symbols) - half))


def codes_of(tab):
    """symbol -> (code, length) of a (counts, symbols) table; of a symbol held twice, the first"""
    counts, symbols = tab
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out.setdefault(symbols[k], (code, length))
            code, k = code + 1, k + 1
        code <<= 1
    return out


# ---- entropy coding ---------------------------------------------------------------------------------------------------------------------------
class Tokens(list):
    """a block given as its symbols, [(symbol, value bits, number of value bits)], the DC's first: written as they stand (damaged forms);
    the predictor is left alone"""


def value_bits(v):
    """(size, the size bits) of a DC difference or an AC coefficient (T.81 F.1.2.1)"""
    s = abs(int(v)).bit_length()
    return s, int(v) if v >= 0 else int(v) + (1 << s) - 1


def block_tokens(coef, pred):
    s, bits = value_bits(int(coef[0]) - pred)
    tokens, run = [(s, bits, s)], 0
    for k in range(1, 64):
        if coef[k] == 0:
            run += 1
            continue
        while run > 15:
            tokens.append((0xF0, 0, 0))
            run -= 16
        s, bits = value_bits(coef[k])
        tokens.append((run << 4 | s, bits, s))
        run = 0
    if run:
        tokens.append((0x00, 0, 0))
    return tokens


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc, self.n = self.acc << n | v, self.n + n
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)                                              # stuffing
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)                       # pad with ones


def encode_scan(blocks, layout, ht, sel, restart=0):
    """the entropy-coded bytes of blocks in scan order (rows of 64 in zigzag order, or ``Tokens``): per MCU the luma blocks, then Cb, Cr.
    RSTn after every ``restart`` MCUs, the predictors reset there."""
    per, lh, lv = MCU[layout]
    luma = lh * lv
    codes = {k: codes_of(t) for k, t in ht.items()}
    assert len(blocks) % per == 0
    w, preds = _Bits(), [0, 0, 0]
    for m in range(len(blocks) // per):
        if restart and m and m % restart == 0:
            w.flush()
            w.out += bytes((0xFF, 0xD0 + (m // restart - 1) % 8))
            preds = [0, 0, 0]
        for j in range(per):
            c = 0 if j < luma else j - luma + 1
            b = blocks[m * per + j]
            if isinstance(b, Tokens):
                tokens = b
            else:
                tokens = block_tokens(b, preds[c])
                preds[c] = int(b[0])
            for i, (sym, bits, n) in enumerate(tokens):
                code, length = codes[(0, sel[c][0]) if i == 0 else (1, sel[c][1])][sym]
                w.put(code, length)
                if n:
                    w.put(bits, n)
    w.flush()
    return bytes(w.out)


# ---- samples to blocks ------------------------------------------------------------------------------------------------------------------------
def _plane_blocks(p, q):
    """a plane whose sides are multiples of 8, level-shifted, as (rows, cols, 64) quantised coefficients in zigzag order"""
    r, c = p.shape[0] // 8, p.shape[1] // 8
    b = (p.astype(np.float64) - 128.0).reshape(r, 8, c, 8).transpose(0, 2, 1, 3)
    d = np.rint((_C @ b @ _C.T).reshape(r, c, 64) / np.asarray(q, dtype=np.float64)).astype(np.int64)
    return d[:, :, ZIGZAG]


def blocks_from_image(img, layout, qts):
    """(H, W, 3) RGB or (H, W) grey uint8 samples as quantised blocks in scan order: float64 colour conversion and DCT, edges replicated to
    whole MCUs, chroma box-averaged.  qts: the components' tables (64, natural order)."""
    per, lh, lv = MCU[layout]
    img = np.asarray(img)
    H, W = img.shape[:2]
    mx, my = -(-W // (8 * lh)), -(-H // (8 * lv))
    pad = ((0, my * 8 * lv - H), (0, mx * 8 * lh - W))
    if layout == "L":
        return _plane_blocks(np.pad(img, pad, mode="edge"), qts[0]).reshape(-1, 64).astype(np.int16)
    r, g, b = (np.pad(img[:, :, k].astype(np.float64), pad, mode="edge") for k in range(3))
    y = 0.299 * r + 0.587 * g + 0.114 * b
    cb, cr = -0.168735892 * r - 0.331264108 * g + 0.5 * b + 128, 0.5 * r - 0.418687589 * g - 0.081312411 * b + 128
    cb, cr = (p.reshape(my * 8, lv, mx * 8, lh).mean(axis=(1, 3)) for p in (cb, cr))
    yb = _plane_blocks(y, qts[0]).reshape(my, lv, mx, lh, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, lv * lh, 64)
    out = np.concatenate([yb, _plane_blocks(cb, qts[1])[:, :, None], _plane_blocks(cr, qts[2])[:, :, None]], axis=2)
    return out.reshape(-1, 64).astype(np.int16)


def check_range(blocks, layout, qts):
    """ValueError for a block whose exact inverse DCT leaves [-384, 383] before the level shift: beyond that libjpeg's range-limit table
    wraps while its SIMD packs saturate, so "Pillow's pixels" is not one thing there"""
    per, lh, lv = MCU[layout]
    for i, b in enumerate(blocks):
        if isinstance(b, Tokens):
            continue
        c = 0 if i % per < lh * lv else i % per - lh * lv + 1
        nat = np.zeros(64)
        nat[ZIGZAG] = np.asarray(b, dtype=np.float64)
        x = _C.T @ (nat * np.asarray(qts[c], dtype=np.float64)).reshape(8, 8) @ _C
        if x.min() < -384 - 1e-9 or x.max() > 383 + 1e-9:                        # (1e-9: the float64 rounding of an exact bound)
            raise ValueError("block %d: its inverse DCT spans [%.1f, %.1f], outside [-384, 383]" % (i, x.min(), x.max()))


# ---- models -----------------------------------------------------------------------------------------------------------------------------------
def model(blocks, H, W, layout, qt, ht, sel, restart=0, ids=None, tq=None, sampling=None):
    """qt: id -> table (64, natural order); tq: the components' quantisation ids (default 0, 1, 1); ids: component ids (default 1, 2, 3);
    sampling: the greyscale component's sampling byte (default 0x11)"""
    per, lh, lv = MCU[layout]
    n = 1 if layout == "L" else 3
    tq = list(tq or (0, 1, 1))[:n]
    ids = list(ids or (1, 2, 3))[:n]
    hv = [(sampling or 0x11) >> 4, (sampling or 0x11) & 15] if layout == "L" else None
    comps = [(ids[c],) + (tuple(hv) if hv else ((lh, lv) if c == 0 else (1, 1))) + (tq[c],) for c in range(n)]
    assert len(blocks) == per * -(-W // (8 * lh)) * -(-H // (8 * lv))
    check_range(blocks, layout, [qt[t] for t in tq])
    return dict(H=H, W=W, comps=comps, qt={k: [int(v) for v in t] for k, t in qt.items()}, ht=dict(ht), sel=[tuple(s) for s in sel][:n], restart=restart,
                scan=encode_scan(blocks, layout, ht, sel, restart))


def from_coefficients(blocks, H, W, layout, qt, ht, sel, restart=0, **kw):
    return model(list(blocks), H, W, layout, qt, ht, sel, restart, **kw)


def from_image(img, layout, qt, ht, sel, restart=0, **kw):
    tq = list(kw.get("tq") or (0, 1, 1))
    H, W = np.asarray(img).shape[:2]
    return model(list(blocks_from_image(img, layout, [qt[t] for t in tq])), H, W, layout, qt, ht, sel, restart, **kw)


def _walk(data):
    """([(marker, body)] up to and including SOS, where the entropy-coded data begins)"""
    assert data[:2] == b"\xff\xd8"
    pos, out = 2, []
    while True:
        assert data[pos] == 0xFF, "byte %d is no marker" % pos
        while data[pos] == 0xFF:
            pos += 1
        m, length = data[pos], data[pos + 1] << 8 | data[pos + 2]
        out.append((m, data[pos + 3:pos + 1 + length]))
        pos += 1 + length
        if m == 0xDA:
            return out, pos


def layout_of(m):
    if len(m["comps"]) == 1:
        return "L"
    return {(2, 2): "4:2:0", (2, 1): "4:2:2", (1, 1): "4:4:4"}[m["comps"][0][1:3]]


def parse(data):
    """a baseline file as a model; its scan bytes (fill bytes inside them included) stay as they are.  A table defined twice: the later."""
    data = bytes(data)
    segs, pos = _walk(data)
    m = dict(qt={}, ht={}, restart=0)
    for marker, body in segs:
        at = 0
        if marker == 0xDB:
            while at < len(body):
                nat = [0] * 64
                for k in range(64):
                    nat[ZIGZAG[k]] = body[at + 1 + k]
                m["qt"][body[at] & 15] = nat
                at += 65
        elif marker == 0xC4:
            while at < len(body):
                n = sum(body[at + 1:at + 17])
                m["ht"][body[at] >> 4, body[at] & 15] = (bytes(body[at + 1:at + 17]), bytes(body[at + 17:at + 17 + n]))
                at += 17 + n
        elif marker == 0xDD:
            m["restart"] = body[0] << 8 | body[1]
        elif marker == 0xC0:
            m["H"], m["W"] = body[1] << 8 | body[2], body[3] << 8 | body[4]
            m["comps"] = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(body[5])]
        elif marker == 0xDA:
            m["sel"] = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(body[0])]
    end = pos
    while True:                                                                 # the first marker that is neither stuffing nor RSTn ends the scan
        end = data.find(b"\xff", end)
        if end < 0:
            end = len(data)
            break
        nxt = end
        while nxt < len(data) and data[nxt] == 0xFF:
            nxt += 1
        if nxt == len(data) or not (data[nxt] == 0 or 0xD0 <= data[nxt] <= 0xD7):
            break
        end = nxt + 1
    m["scan"] = data[pos:end]
    return m


def default_layout(m):
    """libjpeg's order: JFIF, one DQT a table, SOF0, one DHT a table (DC 0, AC 0, DC 1, AC 1), DRI if there are intervals, SOS"""
    return ([("JFIF",)] + [("DQT", [i]) for i in sorted(m["qt"])] + [("SOF",)] + [("DHT", [k]) for k in sorted(m["ht"], key=lambda k: (k[1], k[0]))]
            + ([("DRI",)] if m["restart"] else []) + [("SOS",)])


def _segment(marker, body):
    return bytes((0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255)) + bytes(body)


def serialize(m, layout=None, fill_rst=0, fill_eoi=0):
    """The file of a model.  layout: the segments in order, each one of
        ("JFIF",)  ("ADOBE", transform)  ("COM", body)  ("APP", n, body)  ("SOF",)  ("SOS",)  ("DRI",) or ("DRI", value)
        ("DQT", [id or (id, table), ...])  ("DHT", [(class, id) or ((class, id), (counts, symbols)), ...])   one segment, several tables;
                                                                          a given table instead of the model's: for one a later segment redefines
        ("FILL", n)                                                       n fill bytes (FF) before the next marker
    fill_rst / fill_eoi: fill bytes before every RSTn of the scan and before EOI."""
    out = bytearray(b"\xff\xd8")
    for item in layout or default_layout(m):
        kind = item[0]
        if kind == "FILL":
            out += b"\xff" * item[1]
        elif kind == "JFIF":
            out += _segment(0xE0, b"JFIF\0\1\1\0\0\1\0\1\0\0")
        elif kind == "ADOBE":
            out += _segment(0xEE, b"Adobe\0\x64\0\0\0\0" + bytes((item[1],)))
        elif kind == "COM":
            out += _segment(0xFE, item[1])
        elif kind == "APP":
            out += _segment(0xE0 + item[1], item[2])
        elif kind == "DQT":
            body = bytearray()
            for t in item[1]:
                i, nat = t if isinstance(t, tuple) else (t, m["qt"][t])
                body += bytes((i,)) + bytes(int(nat[ZIGZAG[k]]) for k in range(64))
            out += _segment(0xDB, body)
        elif kind == "DHT":
            body = bytearray()
            for t in item[1]:
                (tc, th), (counts, symbols) = t if isinstance(t[0], tuple) else (t, m["ht"][t])
                body += bytes((tc << 4 | th,)) + bytes(counts) + bytes(symbols)
            out += _segment(0xC4, body)
        elif kind == "DRI":
            v = item[1] if len(item) > 1 else m["restart"]
            out += _segment(0xDD, bytes((v >> 8, v & 255)))
        elif kind == "SOF":
            out += _segment(0xC0, bytes((8, m["H"] >> 8, m["H"] & 255, m["W"] >> 8, m["W"] & 255, len(m["comps"]))) + b"".join(bytes((c, h << 4 | v, q)) for c, h, v, q in m["comps"]))
        elif kind == "SOS":
            out += _segment(0xDA, bytes((len(m["comps"]),)) + b"".join(bytes((c[0], td << 4 | ta)) for c, (td, ta) in zip(m["comps"], m["sel"])) + b"\0\x3f\0")
        else:
            raise ValueError("unknown layout item %r" % (item,))
    scan = m["scan"]
    if fill_rst:
        scan = _RST.sub(lambda r: b"\xff" * fill_rst + r.group(0), scan)        # (an FF of entropy-coded data is followed by 00: FF Dn is a marker)
    return bytes(out) + scan + b"\xff" * fill_eoi + b"\xff\xd9"


# ---- census -----------------------------------------------------------------------------------------------------------------------------------
def decode_scan(m):
    """the model's entropy-coded data by its own tables, bit by bit: (coef (blocks, 64) int16 in zigzag order, the census counts)"""
    per, lh, lv = MCU[layout_of(m)]
    luma = lh * lv
    if len(m["comps"]) == 1:
        lh = lv = 1                                                             # one component: 8 x 8 blocks in raster order whatever its sampling
    mcus = -(-m["W"] // (8 * lh)) * -(-m["H"] // (8 * lv))
    lookup = {k: {(length, code): s for s, (code, length) in codes_of(t).items()} for k, t in m["ht"].items()}
    coef = np.zeros((mcus * per, 64), dtype=np.int16)
    st = dict(selector=sum(td << 2 * c | ta << (2 * c + 1) for c, (td, ta) in enumerate(m["sel"])), blocks=mcus * per, dc_cat_pos=0, dc_cat_neg=0,
              ac_size_pos=0, ac_size_neg=0, ac63_size_pos=0, ac63_size_neg=0, dc_code_min=99, dc_code_max=0, ac_code_min=99, ac_code_max=0, dc_long=0,
              ac_long=0, zrl_chain=0, zrl=0, run15_sized=0, end63=0, eob_only=0, full_blocks=0, lengths={}, stuffed=len(re.findall(b"\xff+\x00", m["scan"])))
    parts = _RST.split(m["scan"])
    st["segments"] = len(parts)
    step = m["restart"] or mcus
    assert len(parts) == -(-mcus // step), "%d intervals for %d MCUs of %d" % (len(parts), mcus, step)
    for p, part in enumerate(parts):
        clean = re.sub(b"\xff+\x00", b"\xff", part)
        acc, left = int.from_bytes(clean, "big"), 8 * len(clean)
        preds = [0, 0, 0]

        def symbol(cls, th):
            nonlocal left
            for length in range(1, 17):
                s = lookup[cls, th].get((length, (acc >> (left - length)) & ((1 << length) - 1))) if left >= length else None
                if s is not None:
                    left -= length
                    k = "dc" if cls == 0 else "ac"
                    st[k + "_code_min"], st[k + "_code_max"] = min(st[k + "_code_min"], length), max(st[k + "_code_max"], length)
                    st[k + "_long"] += length > 9
                    st["lengths"].setdefault("%s%d" % (k, th), set()).add(length)
                    return s
            raise ValueError("no code matches in interval %d" % p)

        def value(s):
            nonlocal left
            left -= s
            assert left >= 0
            v = (acc >> left) & ((1 << s) - 1)
            return v if v >= 1 << (s - 1) else v - (1 << s) + 1

        for mcu in range(p * step, min((p + 1) * step, mcus)):
            for j in range(per):
                c = 0 if j < luma else j - luma + 1
                row = coef[mcu * per + j]
                s = symbol(0, m["sel"][c][0])
                d = value(s) if s else 0
                key = "dc_cat_pos" if d > 0 else "dc_cat_neg"
                st[key] = max(st[key], s)
                preds[c] += d
                row[0] = preds[c]
                k, chain, first = 1, 0, True
                while k < 64:
                    rs = symbol(1, m["sel"][c][1])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            st["eob_only"] += first
                            break
                        k, chain = k + 16, chain + 1
                        st["zrl"] += 1
                        st["zrl_chain"] = max(st["zrl_chain"], chain)
                    else:
                        k, chain = k + r, 0
                        v = value(s)
                        row[k] = v
                        sign = "_pos" if v > 0 else "_neg"
                        st["ac_size" + sign] = max(st["ac_size" + sign], s)
                        st["run15_sized"] += r == 15
                        if k == 63:
                            st["ac63_size" + sign] = max(st["ac63_size" + sign], s)
                            st["end63"] += 1
                        k += 1
                    first = False
                st["full_blocks"] += int((row[1:] != 0).all())
        assert left < 8 and (acc & ((1 << left) - 1)) == (1 << left) - 1, "interval %d does not end in a pad of ones" % p
    st["lengths"] = {k: tuple(sorted(v)) for k, v in st["lengths"].items()}
    return coef, st


def census(data):
    """What a file's entropy-coded data holds, from its bytes and its own tables: selector (bit 2c: component c's DC id, bit 2c + 1: its AC id,
    as the scan header names them), blocks, segments; dc_cat_pos / dc_cat_neg, the largest DC category of a positive / negative difference;
    ac_size_pos / ac_size_neg likewise, and ac63_size_* at coefficient 63; dc_code_min / _max and ac_code_min / _max, the shortest and longest
    code read; dc_long / ac_long, how many codes read had more than 9 bits; lengths, per table ("dc0", "ac1", ...) the code lengths read; zrl, zrl_chain (the longest run of ZRLs); run15_sized, symbols
    with run 15 and a size; end63, blocks whose last symbol lands on coefficient 63 (no EOB); eob_only, blocks whose ACs are one EOB;
    full_blocks, blocks with all 63 ACs non-zero; stuffed, the scan's FF 00."""
    return decode_scan(parse(data))[1]
