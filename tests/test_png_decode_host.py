"""The PNG decoder's host side, on any machine: parser, lowering, conversions, and the whole decoder restated.

``decode_png_host`` -- the chunk walk, the inflate of csrc/mm_inflate.h, the unfilter and the pixel pass restated in numpy / Python in the
kernels' order -- is held to live Pillow on whole frames with ``np.array_equal``: on files Pillow writes (every mode, bit depth and
compression level, the shapes of the issue), on files of the project's own encoder (tests/test_png_host.py's restatement of it), and on
files tests/png_writer.py constructs token by token.  Each constructed case asserts through the restatement's counters what it reached.
For every clean and damaged stream, ``status == 0`` exactly when zlib's raw inflate produces S bytes of the stripped stream without error;
damaged streams must keep every index in range (Python raises otherwise) and leave the untouched bytes zero.  The parser's rejections
name the file; fault copies of the restatement show that the cases catch each fault; the library's descriptor validation is called
through ctypes; and tools/png_inflate_check.cpp, the kernel's own inflate text as a stand-alone program, runs the damaged corpus under
AddressSanitizer and UBSan (CPU only, never loaded into python)."""
import ctypes
import functools
import importlib
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_stream_cases  # noqa: F401  (adds the decoder's case to the stream-order table before its census is collected)
import png_writer as PW
from conftest import ROOT
from test_png_host import png_restated, render_like

PD = importlib.import_module("3d-magic-mirror_amd.png_decode")
N = importlib.import_module("3d-magic-mirror_amd._native")

try:
    from PIL import Image
except ImportError:
    Image = None

needs_pillow = pytest.mark.skipif(Image is None, reason="Pillow is not installed")
MODES = ("L", "RGB", "RGBA")
SHAPES = ((1, 1), (1, 7), (7, 1), (13, 3), (64, 65), (128, 64))
INFLATE_BITS = ~PD.ST_BAD_FILTER


# ---- contents --------------------------------------------------------------------------------------------------------------------------
def blobs(H, W, seed=0):
    """smooth blobs in [0, 1]: compressible enough that zlib emits dynamic blocks"""
    r = np.random.default_rng(1000 * H + W + seed)
    y, x = np.mgrid[:H, :W]
    a = np.zeros((H, W))
    for _ in range(4):
        cy, cx, s = r.uniform(0, H), r.uniform(0, W), r.uniform(2, max(H, W) / 2 + 2)
        a += np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
    return a / a.max()


def save(im, **kw):
    b = io.BytesIO()
    im.save(b, "PNG", **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def pillow_corpus():
    """(name, file) pairs Pillow writes: modes 1, L, P (bits 1, 2, 4, 8; with and without transparency), LA, RGB, RGBA; compress_level 0, 1,
    6, 9 and optimize=True; the issue's shapes; and one 260 x 130 L, whose 34 KB of stream is the only way to a distance of 32768"""
    out = []
    pal = np.random.default_rng(5).integers(0, 256, 768).astype(np.uint8)
    for H, W in SHAPES:
        a = blobs(H, W)
        g = (a * 255).astype(np.uint8)
        rgb = np.stack([g, (a * 100).astype(np.uint8), 255 - g], 2)
        ims = {"1": Image.fromarray(a > 0.5), "L": Image.fromarray(g), "LA": Image.fromarray(np.stack([g, (a > .3).astype(np.uint8) * 200], 2), "LA"),
               "RGB": Image.fromarray(rgb), "RGBA": Image.fromarray(np.concatenate([rgb, ((a > .3) * 77 + 3).astype(np.uint8)[..., None]], 2))}
        for k, (name, im) in enumerate(ims.items()):
            for lvl in ((0, 1, 6, 9) if (H, W) in ((13, 3), (64, 65)) else ((0, 1, 6, 9)[k % 4],)):
                out.append(("%s_%dx%d_l%d" % (name, H, W, lvl), save(im, compress_level=lvl)))
        out.append(("L_%dx%d_opt" % (H, W), save(ims["L"], optimize=True)))
        for bits in (1, 2, 4, 8):
            q = Image.fromarray((a * ((1 << bits) - 1)).astype(np.uint8), "P")
            q.putpalette(pal[:3 << bits].tolist())
            out.append(("P%d_%dx%d" % (bits, H, W), save(q, bits=bits)))
            out.append(("P%d_%dx%d_trns" % (bits, H, W), save(q, bits=bits, transparency=bytes([0, 128]))))
    render = render_like(130, 260)
    out.append(("L_130x260_render", save(Image.fromarray(render[..., 0]))))
    return tuple(out)


def distant_file():
    """the 130 x 260 render-like L file of the corpus"""
    return dict(pillow_corpus())["L_130x260_render"]


def own_corpus():
    """files of the project's own encoder (tests/test_png_host.py restates it byte for byte): fixed-code blocks of independent segments"""
    out = []
    for mode, shapes in (("RGB", ((3, 5), (64, 65))), ("L", ((3, 5), (64, 65))), ("RGBA", ((3, 5), (33, 17)))):
        for H, W in shapes:
            x = render_like(H, W, seed=H)
            frame = x[..., 0] if mode == "L" else x if mode == "RGB" else np.concatenate([x, 255 - x[..., :1]], 2)
            out.append(("own_%s_%dx%d" % (mode, H, W), png_restated(frame[None], mode)[0]))
    return out


# ---- constructed streams: one filtered row, the tokens chosen ---------------------------------------------------------------------------
def simulate(blocks):
    """what the blocks inflate to, by the tokens' own meaning: the test's independent yardstick beside zlib"""
    out = bytearray()
    for b in blocks:
        if b[0] == "stored":
            out += b[1]
            continue
        for t in b[1]:
            if isinstance(t, int):
                out.append(t)
            elif t[0] == "m":
                for _ in range(t[1]):
                    out.append(out[-t[2]])
    return bytes(out)


def emit(blocks, final_last=True):
    d = PW.Deflate()
    for k, b in enumerate(blocks):
        final = final_last and k == len(blocks) - 1
        if b[0] == "stored":
            d.stored(b[1], final)
        elif b[0] == "fixed":
            d.fixed(b[1], final)
        else:
            d.dynamic(b[1], b[2], b[3], final, **(b[4] if len(b) > 4 else {}))
    return d


def one_row_png(stream_bytes, deflate, **kw):
    """an 8-bit grey file of one row whose filtered stream is ``stream_bytes`` (its first byte, the filter type, must be 0..4)"""
    assert stream_bytes[0] <= 4 and 2 <= len(stream_bytes) <= 65536
    return PW.png(len(stream_bytes) - 1, 1, 8, 0, PW.zlib_wrap(deflate), **kw)


def chain_lengths():
    """a complete literal/length code with lengths 1..15: literals 0..13 get 1..14, end-of-block and length symbol 257 get 15"""
    ll = [0] * 258
    for s in range(14):
        ll[s] = s + 1
    ll[256] = ll[257] = 15
    return ll


def noise_bytes(n, seed, first=0):
    return bytes([first]) + bytes(np.random.default_rng(seed).integers(0, 256, n - 1, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def constructed():
    """name -> (file, the bytes its stream inflates to, the counter keys it must reach)"""
    c = {}

    def add(name, blocks, reach, **kw):
        d = emit(blocks)
        c[name] = (one_row_png(simulate(blocks), d.bytes(), **kw), simulate(blocks), reach)

    head = list(noise_bytes(300, 1))
    add("three_types", [("stored", noise_bytes(40, 2)), ("fixed", head[1:60] + [("m", 20, 3), ("m", 9, 57)]),
                        ("dynamic", [0, 1, 2, 3, ("m", 4, 2), 1], [3, 3, 3, 3] + [0] * 252 + [3, 3, 3, 3], [1, 1])],
        [("block", 0), ("block", 1), ("block", 2), ("overlap",)])
    add("eight_alignments", [("fixed", [0])] + [("fixed", [200 + k])for k in range(9)], [("align", k) for k in range(8)])
    add("stored_0_and_65535", [("fixed", [0]), ("stored", b""), ("stored", noise_bytes(65535, 3, 9))], [("stored", 0), ("stored", 65535)])
    add("lengths_of_15", [("dynamic", [0, 1, 2, 13, 12, ("m", 3, 1), 5, ("m", 3, 1)], chain_lengths(), [1])], [("codelen", 15), ("dcodes", 1), ("dist", 1)])
    add("no_distance_code", [("dynamic", [0, 1, 2, 3, 3, 2], [2, 2, 3, 3] + [0] * 252 + [2], [0])], [("dcodes", 0)])
    # every length and distance symbol with its largest extra value, 285, and the named distances, over a history that is not periodic
    toks, made = list(noise_bytes(700, 4)), 700
    while made < 33000:
        toks.append(("m", 258, 699 if made % 2 else 613))
        made += 258
    for i in range(29):
        toks.append(("m", PW.LENGTH_BASE[i] + (1 << PW.LENGTH_EXTRA[i]) - 1, 1 + 37 * i))
    toks.append(("m", 258, 64, 284))                             # length 258 as symbol 284 + 31 is legal too
    for k in range(30):
        toks.append(("m", 3 + k % 5, PW.DIST_BASE[k] + (1 << PW.DIST_EXTRA[k]) - 1))
    for dist, length in ((1, 70), (3, 20), (64, 130), (65, 131), (63, 64), (32768, 258)):
        toks.append(("m", length, dist))
    add("every_symbol", [("fixed", toks)], [("lsym", s) for s in range(257, 286)] + [("dsym", k) for k in range(30)]
        + [("dist", 1), ("dist", 64), ("dist", 65), ("dist", 32768), ("overlap",)])
    # header repeats: 18 and 17 over the unused literals, a 16 that runs from the literal/length lengths into the distance lengths
    ll = [3, 3, 3, 3] + [0] * 252 + [3, 3, 3, 3]
    header = [3, 3, 3, 3, (18, 138), (18, 104), (17, 10), 3, (16, 6), (16, 5)]
    add("header_repeats", [("dynamic", [0, 1, 2, 3, ("m", 3, 2), ("m", 5, 4), ("m", 4, 7)], ll, [3] * 8, dict(header=header))],
        [("rep", 16), ("rep", 17), ("rep", 18), ("rep_cross",)])
    # a match that crosses a row boundary, trailing bytes, data beyond S
    cross = [("fixed", [0, 9, 7, 5, ("m", 28, 4)])]                 # rows of 8 bytes: the period of 4 keeps every filter byte 0
    c["row_crossing"] = (PW.png(7, 4, 8, 0, PW.zlib_wrap(emit(cross).bytes())), simulate(cross), [("rowcross",)])
    blocks = [("fixed", head[:50])]
    c["trailing_bytes"] = (PW.png(49, 1, 8, 0, PW.zlib_wrap(emit(blocks).bytes()) + bytes(range(40))), simulate(blocks), [("trailing",)])      # (behind the Adler-32: Pillow's zlib has ended by then)
    more = [("fixed", head[:50]), ("fixed", head[50:90])]
    c["beyond_S"] = (PW.png(49, 1, 8, 0, PW.zlib_wrap(emit(more).bytes())), simulate(more)[:50], [("block", 1)])
    return c


def filter_files():
    """filters 0-4 on the first row and on later rows, for bpp 1-4 and the sub-byte depths; contents of few values, so Paeth ties abound"""
    out = []
    rng = np.random.default_rng(11)
    for ctype, depth, ch in ((0, 8, 1), (4, 8, 2), (2, 8, 3), (6, 8, 4), (0, 1, 1), (0, 2, 1), (3, 4, 1)):
        for f0 in range(5):
            hi = min(4, 1 << depth)
            a = rng.integers(0, hi, (6, 9) if ch == 1 else (6, 9, ch)).astype(np.uint8) * (1 if depth < 8 else 61)
            kw = dict(plte=bytes(rng.integers(0, 256, 48, dtype=np.uint8))) if ctype == 3 else {}
            out.append(("filter_t%d_d%d_first%d" % (ctype, depth, f0), PW.png_of(a, depth, ctype, [f0, 0, 1, 2, 3, 4], **kw)))
    return out


def conversion_files():
    """every colour type and depth, palettes with a tRNS shorter than the palette, grey and RGB with a tRNS (ignored outside RGBA)"""
    out = []
    rng = np.random.default_rng(12)
    for ctype, depth, ch in ((0, 1, 1), (0, 2, 1), (0, 4, 1), (0, 8, 1), (3, 1, 1), (3, 2, 1), (3, 4, 1), (3, 8, 1), (4, 8, 2), (2, 8, 3), (6, 8, 4)):
        a = rng.integers(0, 1 << depth, (5, 11) if ch == 1 else (5, 11, ch)).astype(np.uint8)
        kw = {}
        if ctype == 3:
            kw = dict(plte=bytes(rng.integers(0, 256, 3 << depth, dtype=np.uint8)), trns=bytes(rng.integers(0, 256, max(1, (1 << depth) // 2), dtype=np.uint8)))
        out.append(("conv_t%d_d%d" % (ctype, depth), PW.png_of(a, depth, ctype, (4, 1, 3), **kw)))
    return out


def trns_ignored_files():
    rng = np.random.default_rng(13)
    return [("grey_trns", PW.png_of(rng.integers(0, 256, (4, 6)).astype(np.uint8), 8, 0, trns=b"\0\x07")),
            ("rgb_trns", PW.png_of(rng.integers(0, 256, (4, 6, 3)).astype(np.uint8), 8, 2, trns=b"\0\x07\0\x08\0\x09"))]


def clean_corpus(mode="L"):
    """(name, file) of everything clean that decodes in ``mode``"""
    out = list(pillow_corpus()) if Image is not None else []
    out += own_corpus() + [(k, v[0]) for k, v in constructed().items()] + filter_files() + conversion_files()
    if mode != "RGBA":
        out += trns_ignored_files()
    return out


# ---- the judges -----------------------------------------------------------------------------------------------------------------------
def stream_of(file):
    h = PD.parse_png(file)
    ch = PD.CHANNELS_IN[h["ctype"]]
    return h["idat"][2:], h["H"] * (1 + (h["W"] * ch * h["depth"] + 7) // 8)


def zlib_accepts(stream, S):
    """zlib's raw inflate produces S bytes of ``stream`` without error, whatever follows them: fed a byte at a time and stopped at S bytes,
    so that what lies behind the S bytes is never looked at"""
    d, made = zlib.decompressobj(-15), 0
    try:
        for k in range(len(stream)):
            made += len(d.decompress(stream[k:k + 1], S - made))
            if made >= S:
                return True
            if d.eof:
                return False
    except zlib.error:
        return False
    return False


def host(files, mode="L", counters=None, **kw):
    return PD.decode_png_host([f for _, f in files] if files and isinstance(files[0], tuple) else files, mode, counters, **kw)


# ---- the helper's own test ----------------------------------------------------------------------------------------------------------------
def test_every_clean_stream_of_the_writer_inflates_with_zlib():
    for name, (file, want, _) in constructed().items():
        stream, S = stream_of(file)
        assert S == len(want), name
        got = zlib.decompressobj(-15).decompress(stream, S)
        assert got == want, name
    d = PW.Deflate().stored(b"abc").fixed([1, 2, ("m", 3, 1)]).dynamic([0, ("m", 3, 1)], chain_lengths(), [1], final=True)
    assert zlib.decompress(PW.zlib_wrap(d.bytes())) == b"abc" + bytes([1, 2, 2, 2, 2]) + bytes(4)
    assert [m[1] for m in d.marks] == ["stored", "fixed", "dynamic"]
    a = np.random.default_rng(0).integers(0, 256, (7, 5, 3)).astype(np.uint8)
    for f in range(5):
        raw = zlib.decompress(PD.parse_png(PW.png_of(a, 8, 2, (f,), splits=(3, 3, 9), extra=((b"tEXt", b"k\0v"),)))["idat"])
        assert raw[::16] == bytes([f] * 7)
        if Image is not None:
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(PW.png_of(a, 8, 2, (f,))))), a)


# ---- against Pillow -----------------------------------------------------------------------------------------------------------------------
@needs_pillow
@pytest.mark.parametrize("mode", MODES)
def test_whole_frames_equal_pillows(mode):
    files = clean_corpus(mode)
    frames, status = host(files, mode)
    assert not status.any()
    for (name, f), got in zip(files, frames):
        want = np.asarray(Image.open(io.BytesIO(f)).convert(mode))
        assert got.dtype == np.uint8 and np.array_equal(got, want), (mode, name)


@needs_pillow
def test_pillow_corpus_reaches_dynamic_blocks_and_noise_does_not():
    c = {}
    host(list(pillow_corpus()), "L", c)
    assert c["block", 2] > 20 and c["block", 0] > 5 and c["block", 1] > 0
    noise = Image.fromarray(np.random.default_rng(1).integers(0, 256, (64, 65), dtype=np.uint8))
    for kw in (dict(compress_level=1), dict(compress_level=6), dict(compress_level=9), dict(optimize=True)):
        c = {}
        f = save(noise, **kw)
        frames, status = host([f], "L", c)
        assert set(k for k in c if k[0] == "block") == {("block", 0)} and not status.any()      # uniform noise: every strategy falls back to stored blocks
        assert np.array_equal(frames[0], np.asarray(noise))
    c = {}
    host([distant_file()], "L", c)
    assert max(k[1] for k in c if k[0] == "dist") > 16384                      # the long file reaches the far half of the window


def test_own_encoders_files_decode_to_their_frames():
    for mode, shapes in (("RGB", ((3, 5), (64, 65))), ("L", ((3, 5), (64, 65))), ("RGBA", ((3, 5), (33, 17)))):
        for H, W in shapes:
            x = render_like(H, W, seed=H)
            frame = x[..., 0] if mode == "L" else x if mode == "RGB" else np.concatenate([x, 255 - x[..., :1]], 2)
            c = {}
            frames, status = host(png_restated(frame[None], mode), mode, c)
            assert not status.any() and np.array_equal(frames[0], frame) and set(k for k in c if k[0] == "block") == {("block", 1)}


# ---- what the constructed cases reach ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(constructed()))
def test_constructed_case_reaches_what_it_is_named_for(name):
    file, want, reach = constructed()[name]
    c = {}
    low = PD.lower_png_decode([file])
    frames, status = PD.decode_png_host(low, counters=c)
    assert status.tolist() == [0]
    H, W = low["sizes"][0]
    assert np.array_equal(frames[0], np.frombuffer(want, dtype=np.uint8).reshape(H, W + 1)[:, 1:])          # (every filter byte of these is 0)
    for key in reach:
        assert c.get(key), (name, key, sorted(k for k in c if k[0] == key[0]))


def test_idat_splits_at_every_byte_and_empty_chunks():
    a = (blobs(9, 7) * 255).astype(np.uint8)
    whole = PW.png_of(a, 8, 0, (1, 4))
    idat = PD.parse_png(whole)["idat"]
    files = [PW.png(7, 9, 8, 0, idat, splits=(k,)) for k in range(len(idat) + 1)]
    files += [PW.png(7, 9, 8, 0, idat, splits=tuple(range(1, len(idat)))), PW.png(7, 9, 8, 0, idat, splits=(0, 0, 5, 5, 5, len(idat))),
              PW.png(7, 9, 8, 0, idat, extra=((b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"a\0b")), after=((b"tIME", bytes(7)),))]
    frames, status = host(files)
    assert not status.any() and all(np.array_equal(f, a) for f in frames)
    low = PD.lower_png_decode(files)
    assert all(bytes(low["data"][b:e]) == idat[2:] for b, e in low["files"][:, PD.F_BEGIN:PD.F_END + 1])


def test_filters_and_paeth_ties_are_reached():
    c = {}
    frames, status = host(filter_files(), "L", c)
    assert not status.any()
    for bpp in (1, 2, 3, 4):
        for ft in range(5):
            assert c.get(("filter", ft, True, bpp)) and c.get(("filter", ft, False, bpp)), (ft, bpp)
    assert c.get(("paeth_tie", "ab")) and c.get(("paeth_tie", "ac")) and c.get(("paeth_tie", "bc"))


def test_conversion_tables_are_deduplicated_and_what_the_issue_says():
    files = [f for _, f in conversion_files()]
    low = PD.lower_png_decode(files + files, "RGBA")
    assert low["conv"].shape == (8, 256) and (low["files"][:11, PD.F_TABLE] == low["files"][11:, PD.F_TABLE]).all()
    assert sorted(low["files"][:11, PD.F_TABLE].tolist()) == [-1, -1, -1] + list(range(8))
    for depth, scale in ((1, 255), (2, 85), (4, 17), (8, 1)):
        t = PD.conversion_table(0, depth, None, None, "RGBA")
        assert [int(v) for v in t[:1 << depth]] == [v * scale * 0x010101 | 255 << 24 for v in range(1 << depth)]
    t = PD.conversion_table(3, 2, bytes([10, 20, 30, 200, 100, 50]), bytes([7]), "RGBA")
    assert [int(v) for v in t[:4]] == [10 | 20 << 8 | 30 << 16 | 7 << 24, 200 | 100 << 8 | 50 << 16 | 255 << 24, 255 << 24, 255 << 24]
    assert int(PD.conversion_table(3, 2, bytes([10, 20, 30, 200, 100, 50]), None, "L")[1]) == (19595 * 200 + 38470 * 100 + 7471 * 50 + 32768) >> 16
    assert low["workspace_bytes"] == N.up256(low["stream_bytes"]) + N.up256(4 * low["n"]) and low["offsets"][-1] == 2 * 11 * 55


# ---- acceptance against zlib, range and zero checks on damaged streams -----------------------------------------------------------------
def small_file():
    return PW.png_of((blobs(13, 3) * 255).astype(np.uint8), 8, 0, (0, 1, 2, 3, 4))


def rewrap(file, stream):
    """``file`` with its deflate data replaced (the CRCs are computed over whatever bytes there are, so the parser passes)"""
    h = PD.parse_png(file)
    return PW.png(h["W"], h["H"], h["depth"], h["ctype"], h["idat"][:2] + stream)


def bad(d):
    return PW.png(19, 1, 8, 0, b"\x78\x01" + d.bytes())


@functools.lru_cache(maxsize=None)
def damaged_corpus():
    """(name, file, the status bit it is made for or None)"""
    out = []
    base = small_file()
    stream, _ = stream_of(base)
    out += [("trunc_%d" % k, rewrap(base, stream[:k]), None) for k in range(len(stream))]
    for bit in range(8 * min(64, len(stream))):
        s = bytearray(stream)
        s[bit >> 3] ^= 1 << (bit & 7)
        out.append(("flip_%d" % bit, rewrap(base, bytes(s)), None))
    D, ll8 = PW.Deflate, [3, 3, 3, 3] + [0] * 252 + [3, 3, 3, 3]
    lit = [0] + list(range(1, 20))
    out += [
        ("ends_behind_a_stored_block", bad(D().fixed(lit[:5]).stored(b"")), PD.ST_OVERRUN),
        ("all_zero_lengths", bad(D().fixed(lit[:5]).dynamic([], [], [], end=False)), PD.ST_BAD_TABLE),
        ("bad_block_btype3", PW.png(19, 1, 8, 0, b"\x78\x01" + bytes([0b110])), PD.ST_BAD_BLOCK),
        ("bad_block_nlen", bad(D().stored(bytes(20), True, nlen=0x1234)), PD.ST_BAD_BLOCK),
        ("bad_code_286", bad(D().fixed(lit[:5] + [("ll", 286)] + lit[5:], True)), PD.ST_BAD_CODE),
        ("bad_code_d30", bad(D().fixed(lit[:5] + [("ll", 257), ("d", 30, 0)] + lit[5:], True)), PD.ST_BAD_CODE),
        ("bad_code_unassigned", bad(D().dynamic([("bits", 1, 1)], [0] * 256 + [1], [0], True, end=False)), PD.ST_BAD_CODE),
        ("bad_distance", bad(D().fixed(lit[:3] + [("m", 3, 4)] + lit, True)), PD.ST_BAD_DISTANCE),
        ("short", bad(D().fixed(lit[:12], True)), PD.ST_SHORT),
        ("short_stored", bad(D().stored(bytes(12), True)), PD.ST_SHORT),
        ("overrun_stored", PW.png(19, 1, 8, 0, b"\x78\x01" + D().stored(bytes(30), True).bytes()[:10]), PD.ST_OVERRUN),
        ("cl_oversubscribed", bad(D().dynamic(lit[:4], ll8, [1, 1], True, cl_lens=[1, 1, 0, 1] + [0] * 15)), PD.ST_BAD_TABLE),
        ("cl_incomplete", bad(D().dynamic(lit[:4], ll8, [1, 1], True, cl_lens=[2, 2, 0, 2] + [0] * 15)), PD.ST_BAD_TABLE),
        ("ll_oversubscribed", bad(D().dynamic([], [1, 1, 1] + [0] * 253 + [2], [1, 1], True)), PD.ST_BAD_TABLE),
        ("ll_incomplete", bad(D().dynamic([], [2, 2] + [0] * 254 + [2], [1, 1], True)), PD.ST_BAD_TABLE),
        ("dd_oversubscribed", bad(D().dynamic(lit[:4], ll8, [1, 1, 1], True)), PD.ST_BAD_TABLE),
        ("dd_incomplete", bad(D().dynamic(lit[:4], ll8, [2, 2], True)), PD.ST_BAD_TABLE),
        ("no_end_of_block", bad(D().dynamic([], [1, 1] + [0] * 255, [1, 1], True, end=False)), PD.ST_BAD_TABLE),
        ("repeat_at_the_start", bad(D().dynamic([], ll8, [1, 1], True, header=[(16, 3)] + ll8[3:] + [1, 1])), PD.ST_BAD_TABLE),
        ("repeat_past_the_end", bad(D().dynamic([], ll8, [1, 1], True, header=ll8 + [1, (16, 6)])), PD.ST_BAD_TABLE),
        ("too_many_lengths", bad(D().dynamic([], [8] * 287, [1, 1], True, hlit=287)), PD.ST_BAD_TABLE),
    ]
    f = bytearray(PW.png_of((blobs(5, 4) * 255).astype(np.uint8), 8, 0, (0, 7, 2, 200, 1)))
    out.append(("bad_filter", bytes(f), PD.ST_BAD_FILTER))
    return tuple(out)


def test_status_is_zero_exactly_when_zlib_inflates_S_bytes_clean():
    for mode in ("L",):
        files = clean_corpus(mode)
        _, status = host(files, mode)
        for (name, f), st in zip(files, status.tolist()):
            assert st == 0 and zlib_accepts(*stream_of(f)), name


def test_status_is_zero_exactly_when_zlib_inflates_S_bytes_damaged():
    corpus = damaged_corpus()
    seen = 0
    for name, f, bit in corpus:
        low = PD.lower_png_decode([f])
        streams = np.zeros(low["stream_bytes"] + 64, dtype=np.uint8)
        rec = low["files"][0].tolist()
        S = rec[PD.F_H] * (1 + rec[PD.F_ROWB])
        inf = PD.HostInflate(low["data"].tobytes(), rec[PD.F_BEGIN], rec[PD.F_END], streams, 32, S)      # (an index out of range raises: Python's own check)
        st = inf.run()
        assert (st == 0) == zlib_accepts(*stream_of(f)), (name, st)
        assert 0 <= inf.o <= S and (st == 0) == (inf.o == S) and not streams[:32].any() and not streams[32 + inf.o:].any(), name      # the untouched bytes are zero
        frames, status = host([f])
        assert status[0] & INFLATE_BITS == st and frames[0].shape == tuple(low["sizes"][0])
        if bit is not None:
            assert status[0] & bit, (name, int(status[0]))
        seen |= int(status[0])
    assert seen == 127                                                         # every status bit is reached
    assert sum(1 for n, f, _ in corpus if n.startswith("flip") and host([f])[1][0] == 0) > 0      # some flips only change pixels


# ---- the parser --------------------------------------------------------------------------------------------------------------------------
def test_every_rejection_names_the_file():
    a = (blobs(4, 5) * 255).astype(np.uint8)
    good = PW.png_of(a, 8, 0)
    idat = PD.parse_png(good)["idat"]
    hdr = lambda W=5, H=4, depth=8, ctype=0, lace=0: PW.chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, lace))      # noqa: E731
    tail = PW.chunk(b"IDAT", idat) + PW.chunk(b"IEND", b"")
    S = PW.SIGNATURE
    cases = {
        "no PNG signature": b"\x89PNX" + good[4:],
        "no IHDR": S + tail,
        "no IDAT": S + hdr() + PW.chunk(b"IEND", b""),
        "not consecutive": S + hdr() + PW.chunk(b"IDAT", idat[:5]) + PW.chunk(b"tEXt", b"a\0b") + PW.chunk(b"IDAT", idat[5:]) + PW.chunk(b"IEND", b""),
        "bad CRC": S + hdr() + PW.chunk(b"IDAT", idat, crc=1) + PW.chunk(b"IEND", b""),
        "runs past the file": good[:-20],
        "16-bit": S + hdr(depth=16) + tail,
        "Adam7": S + hdr(lace=1) + tail,
        "does not allow": S + hdr(depth=4, ctype=2) + tail,
        "without a PLTE": S + hdr(ctype=3) + tail,
        "zlib header": PW.png(5, 4, 8, 0, b"\x78\x02" + idat[2:]),
        "zlib header (CM": PW.png(5, 4, 8, 0, b"\x88\x1c" + idat[2:]),
        "zlib header (CM = 8, CINFO <= 7, FCHECK, no FDICT": PW.png(5, 4, 8, 0, b"\x78\x20" + idat[2:]),
        "height of 0": S + hdr(H=0) + tail,
        "width or height of 0": S + hdr(W=0) + tail,
    }
    for why, f in cases.items():
        with pytest.raises(ValueError, match=r"file 1: .*" + why.replace("(", r"\(")):
            PD.lower_png_decode([good, f])
    for _, f in trns_ignored_files():
        with pytest.raises(ValueError, match="file 1: a tRNS chunk on colour type"):
            PD.lower_png_decode([good, f], "RGBA")
        assert PD.lower_png_decode([f], "L")["n"] == PD.lower_png_decode([f], "RGB")["n"] == 1      # in the other modes Pillow ignores it, and so do we
    with pytest.raises(ValueError, match="mode must be"):
        PD.lower_png_decode([good], "P")
    with pytest.raises(ValueError, match="an empty list"):
        PD.lower_png_decode([])
    assert PD.lower_png_decode([good[:-12]])["n"] == 1                        # a missing IEND is tolerated
    bad_ancillary = S + hdr() + PW.chunk(b"tEXt", b"a\0b", crc=3) + tail
    assert PD.lower_png_decode([bad_ancillary])["n"] == 1                     # ancillary chunks are skipped, their CRC not read


# ---- the cases catch each fault ------------------------------------------------------------------------------------------------------
class StaleCopy(PD.HostInflate):
    def copy_match(self, length, dist):                              # the whole match in one step: reads bytes the match itself should have written
        k = min(length, self.S - self.o)
        at = self.base + self.o
        self.out[at:at + k] = self.out[at - dist:at - dist + k].copy()
        self.o += k


class ExtraBitsMisplaced(PD.HostInflate):
    def read_match(self, sym, dd):                                   # the length's extra bits read behind the distance symbol instead of before it
        i = sym - 257
        le = 0 if i < 8 or i == 28 else (i >> 2) - 1
        self.fill()
        d = self.symbol(dd)
        if d < 0 or d > 29:
            return 0, 0, PD.ST_BAD_CODE
        length = (258 if i == 28 else 3 + i if i < 8 else 3 + ((4 + (i & 3)) << le)) + self.bits(le)
        de = 0 if d < 4 else (d >> 1) - 1
        return length, (1 + d if d < 4 else 1 + ((2 + (d & 1)) << de)) + self.bits(de), 0


class RepeatStopsAtTheBoundary(PD.HostInflate):
    def read_lengths(self, total, hlit, cl):                         # the two length tables read as two sequences: a repeat does not carry across
        a, st = PD.HostInflate.read_lengths(self, hlit, hlit, cl)
        if st:
            return a, st
        b, st = PD.HostInflate.read_lengths(self, total - hlit, total, cl)
        return a + b, st


class PaethTieWrong(PD.HostPixels):
    def paeth(self, a, b, c):
        pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
        return c if pc <= pa and pc <= pb else b if pb <= pa else a


class AverageOverflows(PD.HostPixels):
    def average(self, a, b):
        return ((a + b) & 255) >> 1


class LowBitFirst(PD.HostPixels):
    def unpack(self, rows, depth, W):
        bits = np.unpackbits(rows, axis=1, bitorder="little")[:, :W * depth].reshape(rows.shape[0], W, depth)
        return (bits.astype(np.uint32) << np.arange(depth, dtype=np.uint32)).sum(axis=2).astype(np.uint32)


def test_the_cases_catch_each_fault():
    files = [(k, v[0]) for k, v in constructed().items() if k in ("three_types", "every_symbol", "header_repeats")] + filter_files() + conversion_files()
    want, st0 = host(files)
    assert not st0.any()
    for kw in (dict(inflate=StaleCopy), dict(inflate=ExtraBitsMisplaced), dict(inflate=RepeatStopsAtTheBoundary),
               dict(pixels=PaethTieWrong), dict(pixels=AverageOverflows), dict(pixels=LowBitFirst)):
        got, st = host(files, **kw)
        wrong = [name for (name, _), g, w, s in zip(files, got, want, st.tolist()) if s or not np.array_equal(g, w)]
        assert wrong, kw
    assert "header_repeats" in [name for (name, _), s in zip(files, host(files, inflate=RepeatStopsAtTheBoundary)[1].tolist()) if s]


# ---- the C ABI (CPU library build: nothing is launched) --------------------------------------------------------------------------------
def descriptor(low, keep):
    d = N.MMPngDecodeDesc()
    d.n, d.channels, d.n_tables, d.n_bytes = low["n"], low["channels"], low["conv"].shape[0], low["data"].size
    tables = np.ascontiguousarray(low["tables"]).copy()
    keep.append(tables)
    d.tables_host = tables.ctypes.data
    return d, tables


def test_abi_struct_workspace_and_refusals():
    L = N.lib()
    assert L.mm_struct_size(46) == ctypes.sizeof(N.MMPngDecodeDesc) > 0 and N.STRUCT_IDS[46] is N.MMPngDecodeDesc and N.ABI_VERSION == L.mm_abi_version() == 9
    keep = []
    files = [f for _, f in conversion_files()]
    call, query = N.fn("mm_png_decode"), N.fn("mm_png_decode_query_workspace")
    for mode in MODES:
        low = PD.lower_png_decode(files, mode)
        d, _ = descriptor(low, keep)
        assert query(d) == low["workspace_bytes"]
    low = PD.lower_png_decode(files, "RGBA")
    BAD, UNSUP, NULL, WS = -2, -5, -1, -3

    def status(edit=None, **fields):
        d, tables = descriptor(low, keep)
        if edit:
            edit(tables)
        for k, v in fields.items():
            setattr(d, k, v)
        st = call(d, None)
        assert (query(d) == 0) == (st != NULL or not d.tables_host), (st, query(d))
        return st

    def put(at, value):
        return lambda t: t.__setitem__(at, value)

    F, t_off = PD, 16 * low["n"]
    assert status() == NULL                                                    # the tables pass; bytes, tables, out and workspace are NULL
    assert status(n=0) == BAD and status(channels=2) == BAD and status(n_bytes=0) == BAD and status(n_tables=-1) == BAD
    assert status(n_bytes=(1 << 30) + 1) == UNSUP and status(tables_host=None) == NULL
    assert status(put(F.F_H, 0)) == BAD and status(put(F.F_W, 70000)) == UNSUP and status(put(F.F_CTYPE, 5)) == BAD
    assert status(put(F.F_DEPTH, 16)) == UNSUP and status(put(F.F_DEPTH, 3)) == BAD and status(put(16 * 9 + F.F_DEPTH, 4)) == BAD
    assert status(put(F.F_BPP, 2)) == BAD and status(put(F.F_ROWB, 3)) == BAD and status(put(F.F_TABLE, 8)) == BAD and status(put(16 * 9 + F.F_TABLE, 0)) == BAD
    assert status(put(F.F_BEGIN, -1)) == BAD and status(put(F.F_END, low["data"].size + 1)) == BAD and status(put(16 + F.F_SOFF, 1)) == BAD
    assert status(lambda t: (t.__setitem__(16 + F.F_BEGIN, 9), t.__setitem__(16 + F.F_END, 8))) == BAD
    assert status(put(t_off + 2, 1)) == BAD and status(put(t_off, 1)) == BAD
    d, _ = descriptor(low, keep)                                               # a workspace that is too small or misaligned, tables that are misaligned
    d.bytes, d.tables, d.out, d.workspace, d.workspace_bytes = 64, 64, 64, 64, low["workspace_bytes"] - 1
    assert call(d, None) == WS
    d.workspace, d.workspace_bytes = 72, low["workspace_bytes"]
    assert call(d, None) == WS
    d.workspace, d.tables = 64, 68
    assert call(d, None) == WS
    bn = importlib.import_module("3d-magic-mirror_amd.build_native")
    assert bn.SOURCES["mm_png_decode.hip"] == bn.EXACT and "mm_inflate.h" in bn.HEADERS


# ---- damaged streams: the kernel's own inflate text under the host sanitizers -------------------------------------------------------------
def checksum(a):
    with np.errstate(over="ignore"):
        i = np.arange(a.size, dtype=np.uint64)
        return "%016x" % int(((a.astype(np.uint64) + np.uint64(1)) * (i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1))).sum(dtype=np.uint64))


def test_the_kernels_inflate_text_runs_the_corpus_clean_under_the_sanitizers(tmp_path):
    """tools/png_inflate_check.cpp: a stand-alone program, never loaded into python; a plain build that fails is an error, not a skip"""
    exe = str(tmp_path / "png_inflate_check")
    base = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "3d-magic-mirror_amd", "csrc"),
            os.path.join(ROOT, "tools", "png_inflate_check.cpp"), "-o", exe]
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr[-2000:]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("g++ -fsanitize=address,undefined cannot build here: " + r.stderr[-400:])
    files = [f for _, f, _ in damaged_corpus()] + [v[0] for v in constructed().values()] + [f for _, f in own_corpus()]
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    expect = []
    for k, f in enumerate(files):
        stream, S = stream_of(f)
        out = np.zeros(S, dtype=np.uint8)
        st = PD.HostInflate(stream, 0, len(stream), out, 0, S).run()
        expect.append("%d %s" % (st, checksum(out)))
        (corpus / ("%06d.bin" % k)).write_bytes(struct.pack("<I", S) + stream)
    r = subprocess.run([exe, str(corpus)], capture_output=True, text=True)
    assert r.returncode == 0, "the sanitized inflate did not exit clean:\n%s" % r.stderr[-2000:]
    assert r.stdout.splitlines() == expect
