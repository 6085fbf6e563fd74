"""The GIF encoder restated in numpy and plain Python, and judged by Pillow's decoder: no GPU.

``quantize_restated`` and ``gif_restated`` follow the order written in csrc/mm_gif.hip and include/mm_render.h step by step -- histogram,
median cut, indices, LZW in independent segments, sub-blocks, file -- with integers only, so the device is held to them with ``==``
(tests/test_gpu_gif.py).  Here live Pillow judges the restatement: every file opens, has n frames, every frame's ``convert('RGB')`` is
``palette[indices]``, and loop and duration round-trip.

The constructed cases are named for what they reach, and each asserts through the writer's counters that it does: widths 10 and 11 inside a
segment, the extra width bump after a segment's last data code (before a Clear and before EOI), the longest strings, every sub-block edge,
the frame scans.  ``FAULTS`` are switchable mistakes of the same writer; the cases catch each of them (Pillow misreads the file)."""
import functools
import importlib
import io

import numpy as np
import pytest
import torch

G = importlib.import_module("3d-magic-mirror_amd.gif")
S = G.GIF_SEGMENT

try:
    from PIL import Image
except ImportError:
    Image = None

needs_pillow = pytest.mark.skipif(Image is None, reason="Pillow judges the restatement")

FAULTS = ("no_final_bump", "late_width", "len_256", "no_closing_clear", "msb_first")


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def quantize_restated(frames, log=None):
    """(palette (256,3) uint8, indices (n,H,W) uint8) of (n,H,W,3) uint8 frames; log: a list that receives (box, axis, k, lo, hi) per split"""
    f = np.asarray(frames).reshape((-1,) + tuple(np.asarray(frames).shape[-3:])).astype(np.int64)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    bins = (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3)
    flat = bins.reshape(-1)
    count = np.bincount(flat, minlength=32768)
    low = [np.bincount(flat, weights=(c & 7).reshape(-1), minlength=32768).astype(np.int64) for c in (r, g, b)]
    ids = np.nonzero(count)[0]                                           # the non-empty bins
    cnt = count[ids]
    coord = np.stack([(ids >> 10) & 31, (ids >> 5) & 31, ids & 31])      # r, g, b
    box = np.zeros(len(ids), dtype=np.int64)
    boxes = 1
    while boxes < 256:
        total = np.bincount(box, weights=cnt, minlength=boxes).astype(np.int64)          # (exact: the counts stay below 2^29)
        splittable = np.bincount(box, minlength=boxes) >= 2
        if not splittable.any():
            break
        target = int(np.argmax(np.where(splittable, total, -1)))        # the largest pixel count among the boxes of two bins or more; argmax
        best = int(total[target])                                       # takes the first of equals: the lowest index wins a tie
        m = box == target
        ext = [coord[a][m].max() - coord[a][m].min() for a in range(3)]
        axis = 1 if ext[1] >= ext[0] and ext[1] >= ext[2] else (0 if ext[0] >= ext[2] else 2)
        lo, hi = coord[axis][m].min(), coord[axis][m].max()
        half = (best + 1) // 2
        marginal = np.bincount(coord[axis][m], weights=cnt[m], minlength=32).astype(np.int64)
        k, cum = hi - 1, 0
        for c in range(lo, hi):                                          # the smallest coordinate in [lo, hi - 1] whose cumulative count reaches half
            cum += marginal[c]
            if cum >= half:
                k = c
                break
        box[m & (coord[axis] > k)] = boxes
        if log is not None:
            log.append((target, axis, int(k), int(lo), int(hi)))
        boxes += 1
    palette = np.zeros((256, 3), dtype=np.uint8)
    for i in range(boxes):
        m = box == i
        c = int(cnt[m].sum())
        for a in range(3):
            s = int((cnt[m] * (coord[a][m] << 3) + low[a][ids[m]]).sum())
            palette[i, a] = (2 * s + c) // (2 * c)
    lut = np.zeros(32768, dtype=np.uint8)
    lut[ids] = box
    return palette, lut[bins].astype(np.uint8)


def lzw_codes(pixels, first, last, faults=(), counters=None):
    """one segment's (code, width) list: greedy longest match with a fresh dictionary"""
    out = [(256, 9)] if first else []
    table, nxt, width = {}, 258, 9
    late = 1 if "late_width" in faults else 0
    w, run, longest = int(pixels[0]), 1, 1
    for c in pixels[1:]:
        c = int(c)
        hit = table.get((w, c))
        if hit is not None:
            w, run = hit, run + 1
            continue
        out.append((w, width))
        table[(w, c)] = nxt
        if nxt == (1 << width) + late and width < 12:
            width += 1
        nxt += 1
        w, longest, run = c, max(longest, run), 1
    out.append((w, width))
    longest = max(longest, run)
    bumped = False
    if "no_final_bump" not in faults and nxt == (1 << width) + late and width < 12:      # the decoder adds one more entry here
        width += 1
        bumped = True
    if last or "no_closing_clear" not in faults:
        out.append((257 if last else 256, width))
    if counters is not None:
        counters["max_width"] = max(counters.get("max_width", 9), width)
        counters["longest"] = max(counters.get("longest", 0), longest)
        counters["bump_before_" + ("eoi" if last else "clear")] = counters.get("bump_before_" + ("eoi" if last else "clear"), 0) + bumped
        counters["next"] = max(counters.get("next", 0), nxt)
        widths_inside = {wd for _, wd in out[:-1]}
        counters["widths_inside"] = counters.get("widths_inside", set()) | widths_inside
    return out


def frame_stream(indices, segment, faults=(), counters=None):
    """a frame's code stream as bytes: Clear, the segments, LSB first, the last byte zero-padded"""
    px = np.asarray(indices).reshape(-1)
    nseg = (len(px) + segment - 1) // segment
    acc, nbits = 0, 0
    for s in range(nseg):
        for code, width in lzw_codes(px[s * segment:(s + 1) * segment], s == 0, s == nseg - 1, faults, counters):
            if "msb_first" in faults:
                code = int(format(code, "0%db" % width)[::-1], 2)
            acc |= code << nbits
            nbits += width
    return acc.to_bytes((nbits + 7) // 8, "little")


def gif_restated(frames, delay=10, loop=0, segment=S, faults=(), counters=None, quantized=None):
    """the whole file of (n,H,W,3) or (H,W,3) uint8 frames as bytes.  quantized: (palette, indices) if the caller has them already"""
    f = np.asarray(frames.cpu() if torch.is_tensor(frames) else frames)
    f = f.reshape((-1,) + f.shape[-3:])
    n, H, W = f.shape[:3]
    palette, indices = quantize_restated(f) if quantized is None else quantized
    delays = [delay] * n if isinstance(delay, (int, np.integer)) else list(delay)
    u16 = lambda v: int(v).to_bytes(2, "little")                         # noqa: E731
    out = b"GIF89a" + u16(W) + u16(H) + b"\xf7\x00\x00" + palette.tobytes()
    if loop is not None:
        out += b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + u16(loop) + b"\x00"
    block = 256 if "len_256" in faults else 255
    for i in range(n):
        out += b"\x21\xf9\x04\x04" + u16(delays[i]) + b"\x00\x00" + b"\x2c\x00\x00\x00\x00" + u16(W) + u16(H) + b"\x00" + b"\x08"
        stream = frame_stream(indices[i], segment, faults, counters)
        for j in range(0, len(stream), block):
            piece = stream[j:j + block]
            out += bytes((len(piece) & 255,)) + piece
        out += b"\x00"
        if counters is not None:
            counters.setdefault("stream_bytes", []).append(len(stream))
    return out + b"\x3b"


# ---- Pillow as the judge ----------------------------------------------------------------------------------------------------------------
def pillow_reads(data, palette, indices, delay=10, loop=0):
    """None if Pillow reads ``data`` as the frames palette[indices] with these delays and this loop count; else what differs"""
    indices = np.asarray(indices)
    n = indices.shape[0]
    delays = [delay] * n if isinstance(delay, (int, np.integer)) else list(delay)
    try:
        im = Image.open(io.BytesIO(data))
        if getattr(im, "n_frames", 1) != n:
            return "n_frames %r, not %d" % (getattr(im, "n_frames", 1), n)
        for i in range(n):
            im.seek(i)
            got = np.asarray(im.convert("RGB"))
            if got.shape != palette[indices[i]].shape or not np.array_equal(got, palette[indices[i]]):
                return "frame %d differs" % i
            if im.info.get("duration", 0) != 10 * delays[i]:
                return "frame %d: duration %r, not %d" % (i, im.info.get("duration"), 10 * delays[i])
            if im.info.get("loop") != loop:
                return "loop %r, not %r" % (im.info.get("loop"), loop)
    except Exception as e:                                               # a file Pillow cannot decode is misread too
        return "Pillow raised %s: %s" % (type(e).__name__, e)
    return None


def held(frames, delay=10, loop=0, segment=S, counters=None):
    """the restated file of frames, after Pillow has read it as palette[indices]"""
    f = np.asarray(frames)
    f = f.reshape((-1,) + f.shape[-3:])
    q = quantize_restated(f)
    data = gif_restated(f, delay, loop, segment, counters=counters, quantized=q)
    assert data[:6] == b"GIF89a" and data[-1] == 0x3B
    why = pillow_reads(data, q[0], q[1], delay, loop)
    assert why is None, why
    return data


# ---- content ------------------------------------------------------------------------------------------------------------------------------
# 256 colours in 256 different bins: the median cut gives each its own box, so any index sequence over them keeps its structure (which
# pairs repeat) whatever numbers the boxes get, and every pixel is reproduced exactly
COLOURS = np.array([((i >> 4) * 16 + 4, (i & 15) * 16 + 5, 6) for i in range(256)], dtype=np.uint8)


def all_new_pairs(length):
    """symbols in which no consecutive pair repeats: steps of 1 around the 256, then of 3, 5, ...: every code of a segment is one pixel"""
    out, x, d = [], 0, 1
    while len(out) < length:
        for _ in range(256):
            out.append(x)
            x = (x + d) % 256
        d += 2
    return np.array(out[:length], dtype=np.int64)


def noise(length, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=length).astype(np.int64)


def as_frame(symbols, H=1):
    """symbols as an (H, len / H, 3) frame of COLOURS"""
    return COLOURS[np.asarray(symbols)].reshape(H, -1, 3)


def code_count(symbols):
    return len(lzw_codes(symbols, False, True)) - 1                      # the data codes


@functools.lru_cache(maxsize=None)
def ends_on_bump(length, codes):
    """``length`` symbols that code to exactly ``codes`` data codes: all-new pairs, then a flat tail (found by search, None if there is none)"""
    for head in range(1, length + 1):
        s = np.concatenate([all_new_pairs(head), np.full(length - head, 255 if head < 255 else 77, dtype=np.int64)])
        if code_count(s) == codes:
            return s
    return None


@functools.lru_cache(maxsize=None)
def stream_of(nbytes):
    """(symbols of one frame, segment) whose code stream is exactly ``nbytes`` long: noise, then a flat tail, found by search.  In one segment
    every code past the 255th takes 10 bits, which steps over one length in five (509 among them): those are reached with a shorter segment,
    whose closing Clear moves the count by 9."""
    for length in range(max(nbytes * 8 // 10 - 10, 1), nbytes * 8 // 9 + 100):
        for flat in range(0, min(length, 6)):
            s = np.concatenate([noise(length - flat, 1), np.full(flat, 9, dtype=np.int64)])
            for segment in (S, 300, 260):
                if len(frame_stream(s, segment)) == nbytes:
                    return s, segment
    raise AssertionError("no content found for a stream of %d bytes" % nbytes)


def render_like(H=96, W=128, seed=3):
    """shaded textured blobs on white, (H,W,3) uint8: what a render sheet holds"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.full((H, W, 3), 255.0)
    for _ in range(4):
        cy, cx, rad = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.12, 0.25) * min(H, W)
        d2 = ((yy - cy) ** 2 + (xx - cx) ** 2) / rad ** 2
        inside = d2 < 1
        shade = np.sqrt(np.clip(1 - d2, 0, 1))[..., None]
        base = rng.uniform(40, 230, size=3)
        tex = 18 * np.sin(xx / rng.uniform(2, 6) + yy / rng.uniform(2, 6))[..., None] + rng.normal(0, 3, size=(H, W, 3))
        img = np.where(inside[..., None], np.clip(base * (0.35 + 0.65 * shade) + tex, 0, 255), img)
    return img.astype(np.uint8)


# the small constructed cases, shared with the device's test: name -> (frames (n,H,W,3), kwargs of encode_gif)
def _cases():
    c = {}
    c["1x1"] = (as_frame([5]), {})
    c["1x2"] = (as_frame([5, 200]), {})
    c["7x5"] = (render_like(7, 5), {})
    for seg in (S, 512, 2048, 3838):
        for name, length in (("S-1", seg - 1), ("S", seg), ("S+1", seg + 1), ("2S", 2 * seg)):
            c["%s of %d" % (name, seg)] = (as_frame(noise(length, seg) % 7 * 31), {"segment": seg})
    c["all pairs new"] = (as_frame(all_new_pairs(S)), {})
    c["all pairs new, 3838"] = (as_frame(all_new_pairs(3838)), {"segment": 3838})
    c["bump before clear and eoi, 255"] = (as_frame(np.concatenate([all_new_pairs(255)] * 2)), {"segment": 255})
    c["bump before clear and eoi"] = (as_frame(np.concatenate([ends_on_bump(S, 255)] * 2)), {})
    c["bump to 11 before eoi"] = (as_frame(ends_on_bump(S, 767)), {})
    c["flat"] = (as_frame(np.full(2 * S, 3)), {})
    for nbytes in (254, 255, 256, 509, 510, 511):
        symbols, seg = stream_of(nbytes)
        c["stream of %d" % nbytes] = (as_frame(symbols), {"segment": seg})
    for nseg in (257, 513):                                              # more segments in a frame than a workgroup scans in one pass, twice over
        c["%d segments" % nseg] = (as_frame(noise(4 * nseg, nseg) % 7 * 31).reshape(2, 1, 2 * nseg, 3), {"segment": 2})
    for n in (1, 2, 257, 513):
        c["%d frames" % n] = (COLOURS[(np.arange(n * 6) * 7) % 256].reshape(n, 2, 3, 3), {})
    c["delays"] = (COLOURS[np.arange(4 * 6) % 256].reshape(4, 2, 3, 3), {"delay": [1, 20, 300, 65535], "loop": 3})
    c["no loop"] = (COLOURS[np.arange(2 * 6) % 256].reshape(2, 2, 3, 3), {"delay": 7, "loop": None})
    c["loop 65535"] = (as_frame([1, 2, 3]), {"delay": 2, "loop": 65535})
    c["render-like"] = (np.stack([render_like(40, 56, s) for s in (1, 2, 3)]), {})
    return c


CASES = _cases()


def run_case(name, faults=(), counters=None):
    frames, kw = CASES[name]
    frames = frames.reshape((-1,) + frames.shape[-3:])
    q = quantize_restated(frames)
    data = gif_restated(frames, kw.get("delay", 10), kw.get("loop", 0), kw.get("segment", S), faults, counters, q)
    return data, pillow_reads(data, q[0], q[1], kw.get("delay", 10), kw.get("loop", 0))


# ---- the writer -------------------------------------------------------------------------------------------------------------------------
@needs_pillow
@pytest.mark.parametrize("name", list(CASES))
def test_pillow_reads_the_restated_file(name):
    data, why = run_case(name)
    assert why is None, why
    assert data[:6] == b"GIF89a" and data[-1] == 0x3B


def test_cases_reach_what_they_are_named_for():
    def counted(name):
        k = {}
        run_case_without_pillow(name, k)
        return k
    for seg in (S, 512, 2048, 3838):
        for name, nseg in (("S-1", 1), ("S", 1), ("S+1", 2), ("2S", 2)):
            frames, kw = CASES["%s of %d" % (name, seg)]
            assert kw["segment"] == seg and (frames.shape[0] * frames.shape[1] + seg - 1) // seg == nseg
    k = counted("all pairs new")
    assert {9, 10, 11} <= k["widths_inside"] and k["longest"] == 1 and k["next"] == 258 + S - 1
    k = counted("all pairs new, 3838")
    assert {9, 10, 11, 12} <= k["widths_inside"] and k["next"] == 4095 and k["max_width"] == 12      # 4095: the dictionary is as full as it gets
    for name in ("bump before clear and eoi, 255", "bump before clear and eoi"):
        k = counted(name)
        assert k["bump_before_clear"] == 1 and k["bump_before_eoi"] == 1 and k["next"] == 512, (name, k)
    k = counted("bump to 11 before eoi")
    assert k["bump_before_eoi"] == 1 and k["next"] == 1024 and k["max_width"] == 11
    k = counted("flat")
    assert k["longest"] >= 44 and k["bump_before_clear"] == 0              # strings of 1, 2, 3, ... pixels: 44 * 45 / 2 < 1024
    for nbytes in (254, 255, 256, 509, 510, 511):
        assert counted("stream of %d" % nbytes)["stream_bytes"] == [nbytes]
    for n in (257, 513):
        assert len(counted("%d frames" % n)["stream_bytes"]) == n
    for nseg in (257, 513):                                              # two frames: the second one's offsets restart behind a carry
        frames, kw = CASES["%d segments" % nseg]
        assert frames.shape[0] == 2 and (frames.shape[1] * frames.shape[2] + kw["segment"] - 1) // kw["segment"] == nseg
        assert len(counted("%d segments" % nseg)["stream_bytes"]) == 2


def run_case_without_pillow(name, counters):
    frames, kw = CASES[name]
    return gif_restated(frames, kw.get("delay", 10), kw.get("loop", 0), kw.get("segment", S), (), counters)


@needs_pillow
def test_the_cases_catch_each_fault():
    """a writer with one of FAULTS makes a file Pillow misreads in the case constructed for it (and the right writer's file is read: above)"""
    # (the bump before EOI alone cannot be caught by a decoder: the bit the faulty writer leaves out is a zero, as the padding is; the cases
    # that end on it hold the device to the rule through the file's length and bytes)
    catches = {"no_final_bump": ("bump before clear and eoi, 255", "bump before clear and eoi"),
               "late_width": ("all pairs new", "S of %d" % S),
               "len_256": ("stream of 256", "stream of 509", "stream of 510", "stream of 511"),
               "no_closing_clear": ("S+1 of %d" % S, "2S of %d" % S),
               "msb_first": ("1x2", "7x5")}
    assert set(catches) == set(FAULTS)
    for fault, names in catches.items():
        for name in names:
            _, why = run_case(name, (fault,))
            assert why is not None, (fault, name)
    # and a fault changes nothing where its edge is not reached
    assert run_case("stream of 255", ("len_256",))[1] is None and run_case("stream of 254", ("len_256",))[1] is None
    assert run_case("S-1 of %d" % S, ("no_closing_clear",))[1] is None
    assert run_case("flat", ("no_final_bump",))[1] is None


def test_layout_of_a_tiny_file():
    """1 x 1, one colour: every byte by hand.  Clear (9 bits), code 0, EOI: 0x100 | 0 << 9 | 0x101 << 18 = 27 bits = 4 bytes"""
    frame = np.array([[[255, 255, 255]]], dtype=np.uint8)
    data = gif_restated(frame, delay=10, loop=0)
    want = (b"GIF89a\x01\x00\x01\x00\xf7\x00\x00" + b"\xff\xff\xff" + b"\x00" * 765 + b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"
            + b"\x21\xf9\x04\x04\x0a\x00\x00\x00" + b"\x2c\x00\x00\x00\x00\x01\x00\x01\x00\x00" + b"\x08"
            + b"\x04" + (0x100 | 0x101 << 18).to_bytes(4, "little") + b"\x00" + b"\x3b")
    assert data == want
    assert gif_restated(frame, loop=None) == want[:781] + want[800:]


def test_worst_case_sizes_hold():
    """gif.worst_bits is what a segment of all-new pairs codes to, exactly, and nothing codes to more"""
    for length in (1, 2, 254, 255, 256, 767, 768, 1024, 1791, 1792, 2048, 3838):
        bits = sum(w for _, w in lzw_codes(all_new_pairs(length), False, True))
        assert bits == G.worst_bits(length), length
        assert sum(w for _, w in lzw_codes(noise(length, 5), False, False)) <= G.worst_bits(length)
    assert G.workspace_bytes(36, 64, 96) % 256 == 0 and G.workspace_bytes(1, 1, 1, quantize_only=True) == 256 + 32768 * 17


# ---- the quantiser ------------------------------------------------------------------------------------------------------------------------
def bins_frame(items):
    """pixels from (r5, g5, b5, count[, low]) items: count pixels of colour (r5 << 3 | low, g5 << 3 | low, b5 << 3 | low) each"""
    px = []
    for it in items:
        r, g, b, c = it[:4]
        low = it[4] if len(it) > 4 else 0
        px += [(r << 3 | low, g << 3 | low, b << 3 | low)] * c
    return np.array(px, dtype=np.uint8).reshape(1, 1, -1, 3)


def box_of(items):
    """the box each item's pixels received, in the items' order"""
    f = bins_frame(items)
    pal, idx = quantize_restated(f)
    out, at = [], 0
    for it in items:
        out.append(int(idx[0, 0, at]))
        at += it[3]
    return out, pal


def test_quantiser_one_colour():
    pal, idx = quantize_restated(np.full((2, 3, 4, 3), 255, dtype=np.uint8))
    assert (idx == 0).all() and tuple(pal[0]) == (255, 255, 255) and not pal[1:].any()


def test_quantiser_256_bins_are_exact_and_257_share_one_box():
    f = COLOURS.reshape(1, 16, 16, 3)
    pal, idx = quantize_restated(f)
    assert len(np.unique(idx)) == 256 and np.array_equal(pal[idx], f)
    g = np.concatenate([COLOURS, [[250, 250, 250]]]).astype(np.uint8).reshape(1, 1, 257, 3)
    pal, idx = quantize_restated(g)
    err = np.abs(pal[idx].astype(int) - g).reshape(-1, 3).max(axis=1)
    assert len(np.unique(idx)) == 256 and (err > 0).sum() == 2             # two bins share a box, whose mean is neither


def test_quantiser_ties_and_cuts():
    # equal counts: the lower box splits first.  g: 0, 1 | 8, 9 -> {A, B}, {C, D}; then box 0 (B -> 2), then box 1 (D -> 3)
    assert box_of([(0, 0, 0, 1), (0, 1, 0, 1), (0, 8, 0, 1), (0, 9, 0, 1)])[0] == [0, 2, 1, 3]
    # equal extents on r and g: g is cut first (C leaves), then r (B leaves)
    assert box_of([(0, 0, 0, 2), (4, 0, 0, 1), (0, 4, 0, 1)])[0] == [0, 2, 1]
    # equal extents on all three: g, then r, then b
    assert box_of([(0, 0, 0, 3), (4, 0, 0, 1), (0, 4, 0, 1), (0, 0, 4, 1)])[0] == [0, 2, 1, 3]
    # b alone has the extent
    assert box_of([(1, 1, 0, 1), (1, 1, 9, 1)])[0] == [0, 1]
    # a cut at min: the first coordinate holds half already
    log = []
    quantize_restated(bins_frame([(0, 2, 0, 5), (0, 4, 0, 1), (0, 7, 0, 1)]), log)
    assert log[0] == (0, 1, 2, 2, 7)
    # a cut at max - 1: half is reached only at max, so the cut is clamped and both sides keep a bin
    log = []
    boxes, _ = box_of([(0, 0, 0, 1), (0, 3, 0, 1), (0, 5, 0, 10)])
    quantize_restated(bins_frame([(0, 0, 0, 1), (0, 3, 0, 1), (0, 5, 0, 10)]), log)
    assert log[0] == (0, 1, 4, 0, 5) and boxes == [0, 2, 1]


def test_quantiser_mean_rounds_half_up():
    f = np.array([[[0, 0, 0], [1, 0, 0]]], dtype=np.uint8)[None]           # one bin, mean r = 0.5
    pal, idx = quantize_restated(f)
    assert tuple(pal[0]) == (1, 0, 0) and (idx == 0).all()
    f = np.array([[[0, 2, 7], [1, 2, 7], [1, 3, 6], [0, 2, 6]]], dtype=np.uint8)[None]      # means 0.5, 2.25, 6.5
    assert tuple(quantize_restated(f)[0][0]) == (1, 2, 7)


def psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return float("inf") if mse == 0 else 10 * np.log10(255 ** 2 / mse)


@needs_pillow
def test_quantiser_on_a_render_like_frame_beside_pillows(capsys):
    """the reconstruction error on a render-like frame, printed beside Pillow's median cut on the same frame: a figure, not a threshold --
    the quantiser is this project's own.  Recorded on the 96 x 128 frame below (its texture carries noise): ours 41.90 dB, Pillow's method 0 44.68 dB."""
    f = render_like()
    pal, idx = quantize_restated(f[None])
    ours = psnr(pal[idx[0]], f)
    theirs = psnr(np.asarray(Image.fromarray(f).quantize(256, method=0, dither=Image.Dither.NONE).convert("RGB")), f)
    with capsys.disabled():
        print("\nrender-like 96 x 128: ours %.2f dB, Pillow median cut %.2f dB" % (ours, theirs))
    assert np.isfinite(ours) and pal.shape == (256, 3) and pal.dtype == np.uint8 and idx.max() < 256
    assert (pal[idx[0]][f.min(axis=2) == 255] == 255).all()                # a flat white background stays exactly 255


# ---- the refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_anything_is_launched():
    ok = torch.zeros((2, 4, 5, 3), dtype=torch.uint8)
    assert G.check_frames(ok) == (2, 4, 5) and G.check_frames(ok[0]) == (1, 4, 5)
    with pytest.raises(ValueError, match="export_images"):
        G.encode_gif(ok.float())
    with pytest.raises(ValueError, match="export_images"):
        G.quantize_frames(ok.float())
    one = torch.zeros((1,), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"2\*\*29"):                      # by shape alone: the expanded view owns one byte
        G.encode_gif(one.expand(2, 16384, 16384, 3))
    assert G.check_frames(one.expand(2, 16384, 16383, 3)) == (2, 16384, 16383)
    with pytest.raises(ValueError, match="65535"):
        G.encode_gif(one.expand(1, 1, 65536, 3))
    with pytest.raises(ValueError, match="65535"):
        G.encode_gif(one.expand(1, 65536, 1, 3))
    for bad in (-1, 65536, 1.5, True, [1], [1, 2, 3], [1, 65536], "x"):
        with pytest.raises(ValueError, match="delay"):
            G.encode_gif(ok, delay=bad)
    for bad in (-1, 65536, 0.5):
        with pytest.raises(ValueError, match="loop"):
            G.encode_gif(ok, loop=bad)
    for bad in (0, 3839, 2.0):
        with pytest.raises(ValueError, match="segment"):
            G.encode_gif(ok, segment=bad)
    with pytest.raises(ValueError, match="shape"):
        G.encode_gif(torch.zeros((4, 5, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):            # valid arguments, host memory: there is no host path
        G.encode_gif(ok)


def test_abi_has_the_gif_entry_points(pkg):
    import ctypes
    N = pkg._native
    L = N.lib()
    assert L.mm_struct_size(39) == ctypes.sizeof(N.MMGifDesc) > 0 and N.STRUCT_IDS[39] is N.MMGifDesc
    assert {"mm_gif_query_workspace", "mm_gif_file_offset", "mm_gif_encode"} <= set(N.EXPORTS)
    d = N.MMGifDesc()
    d.n, d.H, d.W, d.segment, d.delay, d.loop = 36, 64, 96, S, 10, 0
    assert L.mm_gif_query_workspace(ctypes.byref(d)) == G.workspace_bytes(36, 64, 96) and L.mm_gif_file_offset(ctypes.byref(d)) == G.FILE_OFFSET
    for seg in (1, 2, 255, 512, 2048, 3838):
        d.segment = seg
        assert L.mm_gif_query_workspace(ctypes.byref(d)) == G.workspace_bytes(36, 64, 96, seg)
    d.segment, d.loop = S, -1
    assert L.mm_gif_query_workspace(ctypes.byref(d)) == G.workspace_bytes(36, 64, 96, loop=None)
    d.quantize_only = 1
    assert L.mm_gif_query_workspace(ctypes.byref(d)) == G.workspace_bytes(36, 64, 96, quantize_only=True)
    d.quantize_only = 0
    assert L.mm_gif_encode(ctypes.byref(d), None) == -1                  # MM_ERR_NULL_POINTER: validation comes before any launch
    d.segment = 3839
    assert L.mm_gif_query_workspace(ctypes.byref(d)) == 0 and L.mm_gif_encode(ctypes.byref(d), None) == -2
    d.segment, d.n, d.H, d.W = S, 2, 16384, 16384
    assert L.mm_gif_query_workspace(ctypes.byref(d)) == 0 and L.mm_gif_encode(ctypes.byref(d), None) == -5
    d.n, d.H, d.W, d.delay = 1, 4, 4, 65536
    assert L.mm_gif_encode(ctypes.byref(d), None) == -2
