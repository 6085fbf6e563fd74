"""The PNG encoder restated in numpy and plain Python, and judged by Pillow's decoder and zlib: no GPU.

``png_restated`` follows the order written in csrc/mm_png.hip and include/mm_render.h step by step -- filter, segments, greedy matching,
fixed Huffman codes, zlib framing, chunks -- with integers only, so the device is held to it with ``==`` (tests/test_gpu_png.py).  Here
Pillow and zlib judge the restatement: every file opens with the right mode and size, ``np.asarray`` of it equals the frame,
``zlib.decompress`` of the IDAT is the filtered stream, every chunk's CRC is ``zlib.crc32``'s and no file is longer than ``lower_png``'s
capacity.

The constructed cases are named for what they reach, and each asserts through the writer's counters that it does.  ``FAULTS`` are
switchable mistakes of the same writer; the cases catch each of them (Pillow or zlib misreads the file)."""
import importlib
import io
import zlib

import numpy as np
import pytest
import torch

P = importlib.import_module("3d-magic-mirror_amd.png")
S = P.PNG_SEGMENT
MAXS = P.PNG_MAX_SEGMENT

try:
    from PIL import Image
except ImportError:
    Image = None

needs_pillow = pytest.mark.skipif(Image is None, reason="Pillow judges the restatement")

FAULTS = ("huffman_not_reversed", "extra_msb_first", "paeth_tie", "adler_no_modulo", "bfinal_every_block")

CHANNELS = {"L": 1, "RGB": 3, "RGBA": 4}
COLOUR_TYPE = {"L": 0, "RGB": 2, "RGBA": 6}
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def as_frames(frames, mode):
    """(n,H,W,C) uint8 of frames (...,H,W[,C])"""
    f = np.asarray(frames.cpu() if torch.is_tensor(frames) else frames)
    C = CHANNELS[mode]
    return f.reshape((-1,) + f.shape[-2:] + (1,)) if mode == "L" else f.reshape((-1,) + f.shape[-3:-1] + (C,))


def paeth(a, b, c, faults=(), counters=None):
    """the Paeth predictor of int arrays a, b, c"""
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    if counters is not None:                                             # the two ties whose order shows in the file (a tie of a and b has pc = 0)
        counters["paeth_tie_a_over_c"] = counters.get("paeth_tie_a_over_c", 0) + int(((pa == pc) & (pa <= pb) & (a != c)).sum())
        counters["paeth_tie_b_over_c"] = counters.get("paeth_tie_b_over_c", 0) + int(((pb == pc) & (pa > pb) & (b != c)).sum())
    if "paeth_tie" in faults:                                            # c first
        return np.where((pc <= pa) & (pc <= pb), c, np.where(pb <= pa, b, a))
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filtered_stream(frame, filter="adaptive", faults=(), counters=None):
    """S of one (H,W,C) frame: H rows of the filter type and the filtered bytes"""
    H, W, C = frame.shape
    raw = frame.reshape(H, W * C).astype(np.int64)
    out = bytearray()
    for y in range(H):
        x = raw[y]
        a = np.concatenate([np.zeros(C, dtype=np.int64), x[:-C]])
        b = raw[y - 1] if y > 0 else np.zeros_like(x)
        c = np.concatenate([np.zeros(C, dtype=np.int64), b[:-C]])
        rows = [x, x - a, x - b, x - (a + b) // 2, x - paeth(a, b, c, faults)]
        rows = [r % 256 for r in rows]
        if filter == "adaptive":
            costs = [int(np.where(r < 128, r, 256 - r).sum()) for r in rows]
            t = costs.index(min(costs))                                  # the first of equals: the lowest type wins a tie
            if counters is not None:
                counters["cost_ties"] = counters.get("cost_ties", 0) + (costs.count(min(costs)) > 1)
                counters["cost_ties_row0"] = counters.get("cost_ties_row0", 0) + (y == 0 and costs.count(min(costs)) > 1)
        else:
            t = int(filter)
        if counters is not None:
            counters.setdefault("types", []).append(t)
            if t == 4:
                paeth(a, b, c, (), counters)
            if t == 3:
                counters["average_odd"] = counters.get("average_odd", 0) + int(((a + b) % 2 == 1).sum())
        out.append(t)
        out += bytes(int(v) for v in rows[t])
    return bytes(out)


class Bits:
    """LSB-first bits of one segment"""

    def __init__(self, faults):
        self.acc, self.n, self.faults = 0, 0, faults

    def put(self, value, width):
        self.acc |= value << self.n
        self.n += width

    def huffman(self, code, width):                                      # most significant bit first
        self.put(code if "huffman_not_reversed" in self.faults else int(format(code, "0%db" % width)[::-1], 2), width)

    def extra(self, value, width):                                       # least significant bit first
        if width:
            self.put(int(format(value, "0%db" % width)[::-1], 2) if "extra_msb_first" in self.faults else value, width)

    def symbol(self, v):
        if v < 144:
            self.huffman(0x30 + v, 8)
        elif v < 256:
            self.huffman(0x190 + (v - 144), 9)
        elif v < 280:
            self.huffman(v - 256, 7)
        else:
            self.huffman(0xC0 + (v - 280), 8)


def largest_code(base, value):
    return max(k for k in range(len(base)) if base[k] <= value)


def deflate_segment(seg, final, faults=(), counters=None):
    """one segment as one fixed-Huffman block: (bits as an int, their count)"""
    out = Bits(faults)
    out.put(1 if final or "bfinal_every_block" in faults else 0, 1)
    out.put(1, 1)
    out.put(0, 1)
    e, i, latest = len(seg), 0, {}
    log = counters.setdefault("log", []) if counters is not None else None
    while i < e:
        j = None
        if i + 3 <= e:
            j = latest.get(seg[i:i + 3])
            latest[seg[i:i + 3]] = i
        if j is None:
            out.symbol(seg[i])
            if log is not None:
                log.append(("literal", seg[i]))
            i += 1
            continue
        L, most = 3, min(258, e - i)
        while L < most and seg[j + L] == seg[i + L]:
            L += 1
        k = largest_code(LENGTH_BASE, L)
        out.symbol(257 + k)
        out.extra(L - LENGTH_BASE[k], LENGTH_EXTRA[k])
        k = largest_code(DIST_BASE, i - j)
        out.huffman(k, 5)
        out.extra(i - j - DIST_BASE[k], DIST_EXTRA[k])
        if log is not None:
            log.append(("match", L, i - j, i + L == e and L < 258))      # the last: the segment's end cut it (or the data ended there)
        for p in range(i + 1, i + L):                                    # the bytes inside a match are later positions' predecessors too
            if p + 3 <= e:
                latest[seg[p:p + 3]] = p
        i += L
    out.symbol(256)
    return out.acc, out.n


def chunk(kind, data):
    return len(data).to_bytes(4, "big") + kind + data + zlib.crc32(kind + data).to_bytes(4, "big")


def adler32(data, faults=()):
    s1, s2 = 1, 0
    for d in data:
        s1 += d
        s2 += s1
        if "adler_no_modulo" not in faults:
            s1, s2 = s1 % 65521, s2 % 65521
    return ((s2 << 16) | s1) & 0xFFFFFFFF


def png_restated(frames, mode="RGB", filter="adaptive", segment=None, faults=(), counters=None):
    """the files of frames (...,H,W[,C]) uint8, a list of bytes in row-major order over the leading dimensions"""
    segment = S if segment is None else segment
    f = as_frames(frames, mode)
    n, H, W, C = f.shape
    files = []
    for i in range(n):
        stream = filtered_stream(f[i], filter, faults, counters)
        nseg = (len(stream) + segment - 1) // segment
        pieces, total = [], 0
        for s in range(nseg):
            acc, nbits = deflate_segment(stream[s * segment:(s + 1) * segment], s == nseg - 1, faults, counters)
            pieces.append(np.unpackbits(np.frombuffer(acc.to_bytes((nbits + 7) // 8, "little"), dtype=np.uint8), bitorder="little")[:nbits])
            total += nbits
        deflate = np.packbits(np.concatenate(pieces), bitorder="little").tobytes()      # blocks bit by bit, zero bits up to a byte
        idat = b"\x78\x01" + deflate + adler32(stream, faults).to_bytes(4, "big")
        ihdr = W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes((8, COLOUR_TYPE[mode], 0, 0, 0))
        files.append(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", idat) + chunk(b"IEND", b""))
        if counters is not None:
            counters.setdefault("deflate_bits", []).append(total)
            counters.setdefault("segments", []).append(nseg)
            counters.setdefault("streams", []).append(stream)
            counters.setdefault("file_bytes", []).append(len(files[-1]))
    return files


# ---- Pillow and zlib as the judges ----------------------------------------------------------------------------------------------------
def chunks_of(data):
    """[(type, data, stored crc)] of a PNG file; raises if the framing is broken"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "signature"
    out, at = [], 8
    while at < len(data):
        n = int.from_bytes(data[at:at + 4], "big")
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n], int.from_bytes(data[at + 8 + n:at + 12 + n], "big")))
        at += 12 + n
    assert at == len(data), "bytes behind the last chunk"
    return out


def misread(data, frame, mode, filter="adaptive", with_pillow=True):
    """None if the file is the (H,W,C) frame to every judge; else what differs"""
    try:
        ch = chunks_of(data)
        if [k for k, _, _ in ch] != [b"IHDR", b"IDAT", b"IEND"]:
            return "chunks %r" % [k for k, _, _ in ch]
        for kind, body, crc in ch:
            if zlib.crc32(kind + body) != crc:
                return "CRC of %r" % kind
        H, W, C = frame.shape
        if ch[0][1] != W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes((8, COLOUR_TYPE[mode], 0, 0, 0)):
            return "IHDR"
        if ch[1][1][:2] != b"\x78\x01":
            return "zlib header"
        if zlib.decompress(ch[1][1]) != filtered_stream(frame, filter):
            return "zlib.decompress(IDAT) is not S"
        if with_pillow and Image is not None:
            im = Image.open(io.BytesIO(data))
            if im.mode != mode or im.size != (W, H):
                return "mode %s size %s" % (im.mode, im.size)
            got = np.asarray(im)
            want = frame[..., 0] if mode == "L" else frame
            if got.shape != want.shape or not np.array_equal(got, want):
                return "Pillow reads other pixels"
    except Exception as e:                                               # a file a judge cannot decode is misread too
        return "%s: %s" % (type(e).__name__, e)
    return None


# ---- content ------------------------------------------------------------------------------------------------------------------------------
def noise(shape, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


def unique_trigrams(length):
    """bytes in which no three consecutive ones repeat: groups (1 + g % 200, 1 + g // 200, 255); values 201..254 and 0 stay free"""
    g = np.arange((length + 2) // 3)
    return np.stack([1 + g % 200, 1 + g // 200, np.full_like(g, 255)], axis=1).reshape(-1)[:length].astype(np.uint8)


def stream_case(row, segment=None):
    """a case whose filtered stream is [0] + row: mode L, one row, filter None"""
    row = np.asarray(row, dtype=np.uint8)
    return row.reshape(1, 1, -1), dict(mode="L", filter=0, segment=S if segment is None else segment)


def runs_frame(lengths, width):
    """one row: for each L a run of L + 1 equal bytes (its own value each: a literal, then ONE match of length L at distance 1), zeros behind"""
    row = np.concatenate([np.full(L + 1, 1 + k, dtype=np.uint8) for k, L in enumerate(lengths)])
    assert len(lengths) < 255 and len(row) <= width
    return np.concatenate([row, np.zeros(width - len(row), dtype=np.uint8)])


def distance_frame(D, width, at=40):
    """one row of unique trigrams but for 201, 202, 203 at `at` and again D further: ONE match, at distance D"""
    row = unique_trigrams(width)
    row[at:at + 3] = (201, 202, 203)
    row[at + D:at + D + 3] = (201, 202, 203)
    return row


# every distance code's first distance and the one before it (the last of the code below), as far as a segment of MAXS holds them;
# 1 and 2 need overlap and have cases of their own
DISTANCES = sorted({d for b in DIST_BASE for d in (b - 1, b) if 3 <= d <= MAXS - 44} | {MAXS - 44})      # (a row of MAXS - 1, the first token at 40)


def render_like(H=66, W=130, seed=3):
    """shaded textured blobs on white, (H,W,3) uint8: what a render sheet holds"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.full((H, W, 3), 255.0)
    for _ in range(4):
        cy, cx, rad = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.12, 0.25) * min(H, W)
        d2 = ((yy - cy) ** 2 + (xx - cx) ** 2) / rad ** 2
        shade = np.sqrt(np.clip(1 - d2, 0, 1))[..., None]
        base = rng.uniform(40, 230, size=3)
        tex = 18 * np.sin(xx / rng.uniform(2, 6) + yy / rng.uniform(2, 6))[..., None] + rng.normal(0, 3, size=(H, W, 3))
        img = np.where((d2 < 1)[..., None], np.clip(base * (0.35 + 0.65 * shade) + tex, 0, 255), img)
    return img.astype(np.uint8)


def five_filters():
    """(7,16,3): a row for every filter type to win"""
    rng = np.random.RandomState(5)
    W, C = 16, 3
    f = np.zeros((7, W, C), dtype=np.int64)
    f[0] = rng.randint(0, 2, size=(W, C)) * 255 % 256 * rng.randint(0, 2, size=(W, C))       # 0 and 255: None (Up ties with it on row 0)
    f[1] = (np.arange(W)[:, None] * 9 + np.array([40, 90, 140])) % 256                      # a ramp: Sub
    f[2] = f[1]                                                                              # the row above again: Up
    f[3] = rng.randint(0, 256, size=(W, C))                                                  # noise above the next two
    flat = f[3].reshape(-1)
    avg = np.zeros(W * C, dtype=np.int64)
    for t in range(W * C):
        avg[t] = ((avg[t - C] if t >= C else 0) + flat[t]) // 2                              # Average predicts it exactly
    f[4] = avg.reshape(W, C)
    f[5] = rng.randint(0, 256, size=(W, C))                                                  # noise again: the predictor below takes a, b and c in turn
    b = f[5].reshape(-1)
    pae = np.zeros(W * C, dtype=np.int64)
    for t in range(W * C):
        if t < C:
            pae[t] = (b[t] + 100) % 256                                                      # (with a = c the predictor is b all along the row: Up)
        else:
            pae[t] = int(paeth(np.array(pae[t - C]), np.array(b[t]), np.array(b[t - C])))    # Paeth predicts the rest exactly
    f[6] = pae.reshape(W, C)
    return f.astype(np.uint8)


# the constructed cases, shared with the device's test: name -> (frames, kwargs of encode_png)
def _cases():
    c = {}
    c["1x1 L"] = (np.array([[[77]]], dtype=np.uint8), dict(mode="L"))
    c["1x1 RGB"] = (np.array([[[[1, 200, 143]]]], dtype=np.uint8), dict(mode="RGB"))
    c["1x1 RGBA"] = (np.array([[[[255, 0, 144, 9]]]], dtype=np.uint8), dict(mode="RGBA"))
    c["five filters"] = (five_filters()[None], dict(mode="RGB"))
    c["paeth ties"] = (np.array([[[10, 13], [4, 50]], [[10, 4], [13, 50]]], dtype=np.uint8), dict(mode="L", filter=4))
    c["average floor"] = (np.array([[[10, 13, 200], [5, 51, 7]]], dtype=np.uint8), dict(mode="L", filter=3))
    for t in range(5):
        c["forced filter %d" % t] = (render_like(9, 11, t), dict(mode="RGB", filter=t))
    c["rgba adaptive"] = (np.concatenate([render_like(12, 10, 1), noise((12, 10, 1), 2)], axis=2), dict(mode="RGBA"))
    c["literals 143 144 255"] = stream_case([143, 144, 255, 1, 142, 145, 254])
    c["match lengths 3..258"] = (np.stack([runs_frame([L for L in range(3, 259) if (L - 3) % 5 == k], MAXS - 1) for k in range(5)])[:, None, :],
                                 dict(mode="L", filter=0, segment=MAXS))
    c["run longer than 258"] = stream_case([7] * 600)
    c["distance 1"] = stream_case([9] * 10)
    c["distance 2"] = stream_case([9, 8] * 6)
    c["distance codes"] = (np.stack([distance_frame(D, MAXS - 1) for D in DISTANCES])[:, None, :], dict(mode="L", filter=0, segment=MAXS))
    c["match cut at the segment end"] = stream_case([5] * 200, 64)
    for seg in (64, S):
        for name, stream in (("S-1", seg - 1), ("S", seg), ("S+1", seg + 1), ("S+2", seg + 2), ("2S", 2 * seg)):
            c["%s of %d" % (name, seg)] = stream_case(noise(stream - 1, seg) % 7 * 31, seg)
    c["bits a multiple of 8"] = stream_case([1, 2, 3, 4, 150, 160, 170, 180, 190, 200])
    c["bits no multiple of 8"] = stream_case([1, 2, 3, 4, 5])
    c["three frames"] = (np.stack([np.full((2, 40), 9, dtype=np.uint8), noise((2, 40), 4), noise((2, 40), 5) % 4 * 60]),
                         dict(mode="L", segment=32))
    c["segment 1"] = (render_like(3, 4, 2), dict(mode="RGB", segment=1))
    c["300 segments"] = (noise((2, 1, 599), 6) % 5 * 50, dict(mode="L", filter=0, segment=2))
    c["300 frames"] = (noise((300, 2, 3), 8) % 3 * 100, dict(mode="L"))
    c["leading dimensions"] = (np.stack([render_like(6, 7, s) for s in range(6)]).reshape(2, 3, 6, 7, 3), dict(mode="RGB"))
    c["render-like"] = (render_like(), dict(mode="RGB"))
    c["noise"] = (noise((40, 40, 3), 9), dict(mode="RGB"))
    return c


CASES = _cases()


def run_case(name, faults=(), counters=None, with_pillow=True):
    """(the files, the first judge's complaint or None)"""
    frames, kw = CASES[name]
    mode = kw.get("mode", "RGB")
    files = png_restated(frames, mode, kw.get("filter", "adaptive"), kw.get("segment"), faults, counters)
    f = as_frames(frames, mode)
    for i, data in enumerate(files):
        why = misread(data, f[i], mode, kw.get("filter", "adaptive"), with_pillow)
        if why is not None:
            return files, "file %d: %s" % (i, why)
    return files, None


# ---- the writer -------------------------------------------------------------------------------------------------------------------------
@needs_pillow
@pytest.mark.parametrize("name", list(CASES))
def test_pillow_and_zlib_read_the_restated_files(name):
    frames, kw = CASES[name]
    files, why = run_case(name)
    assert why is None, why
    f = as_frames(frames, kw.get("mode", "RGB"))
    low = P.lower_png(f.shape[1], f.shape[2], kw.get("mode", "RGB"), kw.get("segment"))
    assert len(files) == f.shape[0] and all(len(d) <= low["file_capacity"] for d in files)


def counted(name):
    k = {}
    run_case(name, (), k, with_pillow=False)
    return k


def matches(k):
    return [e for e in k["log"] if e[0] == "match"]


def test_filter_cases_reach_what_they_are_named_for():
    k = counted("five filters")
    assert k["types"][:3] + k["types"][4::2] == [0, 1, 2, 3, 4], k["types"]       # (rows 3 and 5 are the noise the next ones are predicted from)
    assert k["cost_ties_row0"] == 1                                      # row 0: Up is None there, and the lower type is taken
    k = counted("paeth ties")
    assert k["paeth_tie_a_over_c"] >= 1 and k["paeth_tie_b_over_c"] >= 1 and k["types"] == [4] * 4
    k = counted("average floor")
    assert k["average_odd"] >= 2 and k["types"] == [3, 3]
    for t in range(5):
        assert set(counted("forced filter %d" % t)["types"]) == {t}
    for mode in ("L", "RGB", "RGBA"):
        frames, kw = CASES["1x1 " + mode]
        assert as_frames(frames, mode).shape == (1, 1, 1, CHANNELS[mode]) and counted("1x1 " + mode)["streams"][0][0] == 0


def test_stream_cases_reach_what_they_are_named_for():
    k = counted("literals 143 144 255")
    assert k["log"] == [("literal", v) for v in (0, 143, 144, 255, 1, 142, 145, 254)]
    assert k["deflate_bits"] == [3 + 4 * 8 + 4 * 9 + 7]                  # 143 and 142 take 8 bits, 144 takes 9
    k = counted("match lengths 3..258")
    assert {m[1] for m in matches(k)} == set(range(3, 259)) and k["segments"] == [1] * 5
    assert all(len(s) == MAXS for s in k["streams"])                     # a stream of exactly PNG_MAX_SEGMENT bytes in one segment
    assert all(m[2] == 1 for m in matches(k))
    k = counted("run longer than 258")
    assert k["log"] == [("literal", 0), ("literal", 7), ("match", 258, 1, False), ("match", 258, 1, False), ("match", 83, 1, True)]
    assert counted("distance 1")["log"] == [("literal", 0), ("literal", 9), ("match", 9, 1, True)]
    assert counted("distance 2")["log"] == [("literal", 0), ("literal", 9), ("literal", 8), ("match", 10, 2, True)]
    k = counted("distance codes")
    per_frame = [m[2] for m in matches(k)]
    assert per_frame == DISTANCES, per_frame                             # one match a frame, at its distance
    codes = {largest_code(DIST_BASE, d) for d in DISTANCES}
    assert codes == set(range(2, 26)) and all(b in DISTANCES and b - 1 in DISTANCES for b in DIST_BASE if 4 <= b <= 6145)
    assert max(DISTANCES) == MAXS - 44                                   # the largest the case's layout holds: 13 extra bits are beyond a segment
    k = counted("match cut at the segment end")
    assert k["log"][:3] == [("literal", 0), ("literal", 5), ("match", 62, 1, True)] and k["segments"] == [4]
    assert k["streams"][0][63] == k["streams"][0][64] == 5               # the data went on: the segment's end cut the match


def test_segment_cases_reach_what_they_are_named_for():
    for seg in (64, S):
        for name, nseg, last in (("S-1", 1, seg - 1), ("S", 1, seg), ("S+1", 2, 1), ("S+2", 2, 2), ("2S", 2, seg)):
            k = counted("%s of %d" % (name, seg))
            assert k["segments"] == [nseg] and len(k["streams"][0]) == (nseg - 1) * seg + last, (name, seg)
    assert counted("bits a multiple of 8")["deflate_bits"] == [3 + 5 * 8 + 6 * 9 + 7] and (3 + 5 * 8 + 6 * 9 + 7) % 8 == 0
    assert counted("bits no multiple of 8")["deflate_bits"][0] % 8 != 0
    k = counted("three frames")
    assert len(set(k["file_bytes"])) == 3 and all(s > 1 for s in k["segments"])
    k = counted("segment 1")
    assert k["segments"] == [len(k["streams"][0])] and not matches(k)
    assert counted("300 segments")["segments"] == [300, 300] and len(counted("300 frames")["file_bytes"]) == 300
    # BFINAL on the last block only: the first bit of every block, read back out of the stream
    frames, kw = CASES["S+1 of 64"]
    idat = chunks_of(png_restated(frames, **kw)[0])[1][1]
    first = deflate_segment(filtered_stream(as_frames(frames, "L")[0], 0)[:64], False)
    bits = np.unpackbits(np.frombuffer(idat[2:-4], dtype=np.uint8), bitorder="little")
    assert bits[0] == 0 and bits[first[1]] == 1 and tuple(bits[1:3]) == tuple(bits[first[1] + 1:first[1] + 3]) == (1, 0)


@needs_pillow
def test_the_cases_catch_each_fault():
    """a writer with one of FAULTS makes a file Pillow or zlib misreads in the case constructed for it (the right writer's is read: above)"""
    catches = {"huffman_not_reversed": ("1x1 L", "literals 143 144 255"),
               "extra_msb_first": ("match lengths 3..258", "distance codes"),
               "paeth_tie": ("paeth ties",),
               "adler_no_modulo": ("run longer than 258", "noise"),
               "bfinal_every_block": ("S+1 of 64", "three frames")}
    assert set(catches) == set(FAULTS)
    for fault, names in catches.items():
        for name in names:
            _, why = run_case(name, (fault,))
            assert why is not None, (fault, name)
    # and a fault changes nothing where its edge is not reached
    assert run_case("S of 64", ("bfinal_every_block",))[1] is None
    assert run_case("1x1 L", ("adler_no_modulo",))[1] is None and run_case("1x1 L", ("extra_msb_first",))[1] is None
    assert run_case("forced filter 1", ("paeth_tie",))[1] is None


def test_layout_of_a_tiny_file():
    """1 x 1 grey, value 0: every byte by hand.  S = 00 00; block: 1, 1 0, literal 0 (00110000), a match? no: two bytes have no trigram;
    literal 0 again, end-of-block 0000000: 3 + 8 + 8 + 7 = 26 bits"""
    data = png_restated(np.zeros((1, 1), dtype=np.uint8), "L")[0]
    bits = "110" + "00110000" + "00110000" + "0000000"
    deflate = int(bits[::-1], 2).to_bytes(4, "little")
    want = (b"\x89PNG\r\n\x1a\n" + b"\x00\x00\x00\x0dIHDR\x00\x00\x00\x01\x00\x00\x00\x01\x08\x00\x00\x00\x00" + zlib.crc32(b"IHDR\x00\x00\x00\x01\x00\x00\x00\x01\x08\x00\x00\x00\x00").to_bytes(4, "big")
            + b"\x00\x00\x00\x0aIDAT\x78\x01" + deflate + b"\x00\x02\x00\x01" + zlib.crc32(b"IDAT\x78\x01" + deflate + b"\x00\x02\x00\x01").to_bytes(4, "big")
            + b"\x00\x00\x00\x00IEND\xae\x42\x60\x82")
    assert data == want and zlib.decompress(b"\x78\x01" + deflate + b"\x00\x02\x00\x01") == b"\x00\x00"


def test_worst_case_sizes_hold():
    """lower_png's capacity is what a stream of all 9-bit literals takes, exactly, and nothing takes more"""
    for length, seg in ((1, 64), (63, 64), (64, 64), (65, 64), (200, 64), (500, S)):
        row = 144 + (np.arange(length) * 37) % 112                       # 9-bit literals, no trigram twice (37 is odd: a period of 112)
        frames, kw = stream_case(row[:111] if length > 111 else row, seg)
        k = {}
        files = png_restated(frames, counters=k, **kw)
        low = P.lower_png(1, frames.shape[-1], "L", seg)
        assert not matches(k) and len(files[0]) <= low["file_capacity"]
        assert k["deflate_bits"][0] == 10 * low["segs"] + 9 * low["stream_bytes"] - 1       # (the filter byte 0 is an 8-bit literal)
    low = P.lower_png(40, 40, "RGB", 4096)
    assert low["row_bytes"] == 121 and low["stream_bytes"] == 4840 and low["segs"] == 2
    assert low["file_capacity"] == 8 + 25 + 12 + (2 + (20 + 9 * 4840 + 7) // 8 + 4) + 12
    assert low["workspace_bytes"](36) % 256 == 0 and low["files_offset"](36) == 512
    assert len(png_restated(noise((40, 40, 3), 1), segment=4096)[0]) <= low["file_capacity"]  # uniform noise: 1.07 x raw
    assert P.lower_png(40, 40, "RGB", 4096) is low and P.lower_png(40, 40)["segment"] == S                                                     # cached: read, not written


def test_sizes_beside_raw(capsys):
    """the size of a render-like sheet at the three segment lengths, printed: figures, not thresholds -- the files are larger than a serial
    encoder's with dynamic codes by design.  Recorded on the 66 x 130 sheet below: raw 25740 bytes."""
    f = render_like()
    sizes = {seg: len(png_restated(f, segment=seg)[0]) for seg in (1024, 2048, 4096)}
    with capsys.disabled():
        print("\nrender-like 66 x 130 RGB: raw %d, ours %s" % (f.size, sizes))
    assert sizes[4096] <= sizes[2048] <= sizes[1024] < f.size


# ---- the refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_anything_is_launched():
    ok = torch.zeros((2, 4, 5, 3), dtype=torch.uint8)
    n, lead, low, flt = P.check_frames(ok)
    assert (n, lead, flt) == (2, (2,), -1) and (low["H"], low["W"], low["channels"]) == (4, 5, 3)
    assert P.check_frames(ok[0])[:2] == (1, ()) and P.check_frames(ok[..., 0], "L")[:2] == (2, (2,))
    assert P.check_frames(torch.zeros((3, 2, 4, 5, 4), dtype=torch.uint8), "RGBA", 4, 77)[::3] == (6, 4)
    with pytest.raises(ValueError, match="export_images"):
        P.encode_png(ok.float())
    with pytest.raises(ValueError, match="mask"):
        P.encode_png(ok[..., 0].float(), "L")
    for frames, mode in ((ok, "RGBA"), (ok[..., :2], "RGB"), (torch.zeros((5, 3), dtype=torch.uint8), "RGB"), (torch.zeros((4,), dtype=torch.uint8), "L")):
        with pytest.raises(ValueError, match="shape"):
            P.encode_png(frames, mode)
    with pytest.raises(ValueError, match="empty"):
        P.encode_png(torch.zeros((0, 4, 5, 3), dtype=torch.uint8))
    one = torch.zeros((1,), dtype=torch.uint8)
    with pytest.raises(ValueError, match="65535"):                        # by shape alone: the expanded view owns one byte
        P.encode_png(one.expand(1, 1, 65536, 3))
    with pytest.raises(ValueError, match="65535"):
        P.encode_png(one.expand(1, 65536, 1), "L")
    with pytest.raises(ValueError, match="65535"):
        P.lower_png(0, 5)
    for bad in ("rgb", "P", None, 3):
        with pytest.raises(ValueError, match="mode"):
            P.encode_png(ok, bad)
    for bad in (-1, 5, 1.0, True, "paeth", None):
        with pytest.raises(ValueError, match="filter"):
            P.encode_png(ok, filter=bad)
    for bad in (0, MAXS + 1, 2.0, True):
        with pytest.raises(ValueError, match="segment"):
            P.encode_png(ok, segment=bad)
    with pytest.raises(ValueError, match=r"2\*\*31"):                     # 9 / 8 of 2.1e9 bytes
        P.encode_png(one.expand(1, 32768, 65535), "L")
    assert P.lower_png(29000, 65535, "L")["idat_capacity"] <= P.MAX_IDAT
    with pytest.raises(ValueError, match="numpy|tensor"):
        P.encode_png(np.zeros((4, 5, 3), dtype=np.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):            # valid arguments, host memory: there is no host path
        P.encode_png(ok)


def test_batch_is_jpegs(pkg):
    b = P.PngBatch(np.frombuffer(b"abcdef", dtype=np.uint8), [0, 2, 6], (1, 2))
    assert isinstance(b, pkg.JpegBatch) and len(b) == 2 and list(b) == [b"ab", b"cdef"] and b[-1] == b"cdef" and b.shape == (1, 2)
    with pytest.raises(TypeError, match="PngBatch"):
        b["x"]
    with pytest.raises(TypeError, match="a JpegBatch is indexed by an int"):
        pkg.JpegBatch(np.zeros(1, dtype=np.uint8), [0, 1])["x"]
    assert pkg.encode_png is P.encode_png and pkg.PNG_SEGMENT == S and pkg.PNG_MAX_SEGMENT == MAXS and pkg.lower_png is P.lower_png


def test_abi_has_the_png_entry_points(pkg):
    import ctypes
    import os
    import re
    N = pkg._native
    L = N.lib()
    assert L.mm_struct_size(41) == ctypes.sizeof(N.MMPngDesc) > 0 and N.STRUCT_IDS[41] is N.MMPngDesc and N.ABI_VERSION == L.mm_abi_version() == 9
    assert {"mm_png_query_workspace", "mm_png_files_offset", "mm_png_encode"} <= set(N.EXPORTS)
    assert not {31, 34, 36} & set(N.STRUCT_IDS)
    bn = importlib.import_module("3d-magic-mirror_amd.build_native")
    assert bn.SOURCES["mm_png.hip"] == bn.EXACT
    src = open(os.path.join(bn.CSRC, "mm_png.hip")).read()
    assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", src)) and "atomicAdd" not in src       # integer arithmetic only; OR and XOR atomics
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mm_render.h")).read()
    for name, value in (("MM_PNG_SEGMENT", S), ("MM_PNG_MAX_SEGMENT", MAXS), ("MM_PNG_CRC_PIECE", P.PNG_CRC_PIECE), ("MM_ABI_VERSION", 9)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == value
    for name in ("mm_png_query_workspace", "mm_png_files_offset"):
        assert re.search(r"^size_t %s\(const MMPngDesc\* desc\);" % name, hdr, flags=re.M)
    assert re.search(r"^int mm_png_encode\(const MMPngDesc\* desc, mm_stream_t stream\);", hdr, flags=re.M) and "41 MMPngDesc" in hdr
    d = N.MMPngDesc()
    for n, H, W, mode, seg in ((36, 64, 96, "RGB", S), (1, 1, 1, "L", 1), (3, 7, 5, "RGBA", 2), (48, 256, 128, "RGB", 1024), (2, 300, 200, "L", MAXS), (5, 33, 17, "RGB", 2048)):
        low = P.lower_png(H, W, mode, seg)
        d.n, d.H, d.W, d.channels, d.filter, d.segment = n, H, W, low["channels"], -1, seg
        assert L.mm_png_query_workspace(ctypes.byref(d)) == low["workspace_bytes"](n), (n, H, W, mode, seg)
        assert L.mm_png_files_offset(ctypes.byref(d)) == low["files_offset"](n)
    assert L.mm_png_encode(ctypes.byref(d), None) == -1                  # MM_ERR_NULL_POINTER: validation comes before any launch
    assert L.mm_png_encode(None, None) == -1
    for field, bad in (("segment", 0), ("segment", MAXS + 1), ("channels", 2), ("filter", 5), ("filter", -2), ("n", 0)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        assert L.mm_png_query_workspace(ctypes.byref(d)) == 0 and L.mm_png_encode(ctypes.byref(d), None) == -2, (field, bad)
        setattr(d, field, keep)
    d.n, d.H, d.W, d.channels, d.segment = 1, 32768, 65535, 1, S
    assert L.mm_png_query_workspace(ctypes.byref(d)) == 0 and L.mm_png_encode(ctypes.byref(d), None) == -5       # the IDAT could pass 2^31 - 1
    d.H, d.W = 4, 65536
    assert L.mm_png_encode(ctypes.byref(d), None) == -5
