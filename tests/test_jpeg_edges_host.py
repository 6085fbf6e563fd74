"""Constructed inputs that reach each discrete path of the JPEG encoder's parallel entropy coder (csrc/mm_jpeg.hip), on the host, no GPU.

tests/test_jpeg_host.py holds the restatement to Pillow on noise, ramps, flat frames and renders, where reaching a path is luck.  Every
entry of ``CASES`` here is built for paths that the kernels take one at a time: the five ways a block's bits meet the 32-bit words of
``JpegWriter``, one, two and three ZRLs before a coefficient, blocks without EOB and EOB-only blocks, AC category 10 and DC category 11
with both signs, 0xFF at the last byte of a 1024-byte chunk and at the first of the next, in every byte lane of a word and two in a
row, streams that end on a chunk boundary, one byte past it and at every residue mod 4 with and without padding, a last byte that
padding turns into 0xFF, quantiser ties of both signs, colours next to the colour conversion's rounding boundaries, and more than 256
frames.  For every case the restatement's file is Pillow's whole file, and the restatement's counters equal the figures recorded in the
table, EXACTLY: a case that stops reaching its path fails here.  tests/test_gpu_jpeg_edges.py holds the device to the same cases.

Most inputs are grey (R = G = B = v converts to exactly Y = v, Cb = Cr = 128).  After a flat MCU of the same grey a flat MCU codes to
exactly 32 bits (four times 2 + 4 for luma, two times 2 + 2 for chroma), so the width of a frame of one noise MCU followed by grey moves
the end of its stream in steps of four bytes, and grey MCUs BEFORE noise move every 0xFF of the noise the same way.  The seeds and widths
were found by bounded searches off line and are recorded in the builders; nothing is searched at test time.

A run of four 0xFF cannot occur in a stream of these tables: ``test_no_stream_holds_four_ff_in_a_row`` derives 31 as the most 1-bits in
a row from the tables.  Runs of two are pinned (across a chunk boundary); longer ones stay with the noise of the statistical tests.

The mutation check: ``faulty_files`` is a copy of the restatement's quantiser, stream writer and file layout with a ``fault`` switch, one
believable device mistake each.  Every fault must change a file of the case named for it, and change a file exactly where the counter
that stands for it says so."""
import functools
import math

import numpy as np
import pytest

import test_jpeg_host as T
from test_jpeg_host import differ, ff_runs, jpeg_restated, pillow, writer_shapes

J = T.J


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
def grey(v):
    """(...,) values as (...,3) uint8 with R = G = B"""
    v = np.asarray(v)
    return np.repeat(v[..., None], 3, axis=-1).astype(np.uint8)


def block_checkerboard(first):
    """32 x 32: 8-pixel blocks of 0 and 255, the block at the origin ``first``: luma DCs -1024 and 1016, differences -2040, 0, +2040"""
    y, x = np.mgrid[0:32, 0:32]
    return grey(np.where((y // 8 + x // 8) % 2 == 0, first, 255 - first))


def chroma_checkerboard():
    """32 x 32: 16-pixel MCUs of blue and yellow: Cb is 255 and 0, its DCs 1016 and -1024, the chroma DC differences -2040 and +2040"""
    y, x = np.mgrid[0:32, 0:32]
    blue = ((y // 16 + x // 16) % 2 == 0)[..., None]
    return np.where(blue, np.array([0, 0, 255]), np.array([255, 255, 0])).astype(np.uint8)


def stripes(axis):
    """16 x 16 one-pixel stripes of 0 and 255 along ``axis``: an AC coefficient of -924, category 10"""
    return grey(np.indices((16, 16))[axis] % 2 * 255)


def pixel_checkerboard():
    """16 x 16 one-pixel checkerboard: coefficient 63 is -838, among 17 non-zero ones"""
    y, x = np.mgrid[0:16, 0:16]
    return grey((y + x) % 2 * 255)


def basis77(amplitude=60):
    """the 8 x 8 block 128 + A cos((2y+1) 7 pi / 16) cos((2x+1) 7 pi / 16), normalised to a peak of A: coefficient 63 alone"""
    c = np.cos((2 * np.arange(8) + 1) * 7 * math.pi / 16)
    b = np.outer(c, c)
    return np.round(128 + amplitude * b / np.abs(b).max()).astype(np.int64)


def long_runs():
    """two 16 x 16 frames: the basis block in every luma block; the basis block in Y00 and Y10 with flat 128 in Y01 and Y11"""
    tiled = np.tile(basis77(), (2, 2))
    mixed = tiled.copy()
    mixed[:, 8:] = 128
    return np.stack([grey(tiled), grey(mixed)])


def grey_noise(seed, mcus=1, binary=False):
    """(16,16 mcus,3): grey noise, 0..255 or only 0 and 255"""
    g = np.random.default_rng(seed)
    return grey(g.integers(0, 2, (16, 16 * mcus)) * 255 if binary else g.integers(0, 256, (16, 16 * mcus)))


def noise_then_grey(seed, W, v=90):
    """16 x W: one MCU of grey noise, then flat grey: the width sets the stream's length in steps of 4 bytes"""
    f = np.full((16, W, 3), v, dtype=np.uint8)
    f[:, :16] = grey_noise(seed)
    return f


def grey_then_noise(seed, W, mcus=2, v=90, binary=True):
    """16 x W: flat grey, then ``mcus`` MCUs of noise: the width moves every byte of the noise in steps of 4 bytes"""
    f = np.full((16, W, 3), v, dtype=np.uint8)
    f[:, W - 16 * mcus:] = grey_noise(seed, mcus, binary)
    return f


def writer_mix(seed=4):
    """16 x 192: noise MCUs at 0, 3, 6 and 9 between flat ones, whose 6- and 4-bit blocks lie many to a word at four alignments"""
    f = np.full((16, 192, 3), 90, dtype=np.uint8)
    g = np.random.default_rng(seed)
    for m in (0, 3, 6, 9):
        f[:, 16 * m:16 * m + 16] = grey(g.integers(0, 256, (16, 16)))
    return f


def colour_sums():
    """the three fixed-point sums of the colour conversion before their >> 16, for all 2^24 colours (index R << 16 | G << 8 | B), int32"""
    v = np.arange(256, dtype=np.int32)
    r, g, b = v[:, None, None], v[None, :, None], v[None, None, :]
    return ((19595 * r + 38470 * g + 7471 * b + 32768).reshape(-1),
            (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767).reshape(-1),
            (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767).reshape(-1))


@functools.lru_cache(maxsize=None)
def boundary_colours():
    """(256,3) uint8: the 8 corners of the colour cube, then 248 colours whose Y, Cb or Cr sum lies nearest a multiple of 65536: for each
    of the three sums and each side (just at or above a multiple: the result has just gone up; just below: it is about to), the colours
    in order of distance, ties by colour index; the six lists are dealt in turn until 248 new colours are out"""
    corners = [r << 16 | g << 8 | b for r in (0, 255) for g in (0, 255) for b in (0, 255)]
    index = np.arange(1 << 24, dtype=np.int64)
    lists = []
    for s in colour_sums():
        above = (s & 0xFFFF).astype(np.int64)
        for dist in (above, 0xFFFF - above):
            key = dist << 24 | index
            lists.append(np.sort(np.partition(key, 300)[:300]) & 0xFFFFFF)
    out, rank = list(corners), 0
    while len(out) < 256:
        for l in lists:
            if len(out) < 256 and int(l[rank]) not in out:
                out.append(int(l[rank]))
        rank += 1
    c = np.array(out)
    return np.stack([c >> 16, c >> 8 & 255, c & 255], axis=-1).astype(np.uint8)


def colour_mcus():
    """256 x 256: 256 flat 16 x 16 MCUs, each one of ``boundary_colours``"""
    c = boundary_colours().reshape(16, 16, 3)
    return np.repeat(np.repeat(c, 16, axis=0), 16, axis=1)


def many_frames(n=257):
    """(n,8,8,3) noise: more frames than one pass of the file-offset scan"""
    return np.random.default_rng(n).integers(0, 256, (n, 8, 8, 3), dtype=np.uint8)


def single(f):
    return f[None]


# ---- the cases: name -> (frames (n,H,W,3), quality, the figures of ``measured`` it exists for, exactly) ----------------------------------
# seeds 10, 11, 14, 17: streams that end without padding at the residues 0, 2, 3, 1 mod 4; seeds 0, 3, 1, 4: with padding, at 0, 1, 2, 3
ENDS = (10, 11, 14, 17, 0, 3, 1, 4)
CASES = {
    "dc_extremes": (lambda: np.stack([block_checkerboard(0), block_checkerboard(255), chroma_checkerboard()]), 100, dict(
        first_dc=[-1024, 1016, -792], dc11=[[9, 10], [1, 1]], dc_cat_max=[11, 11])),
    "ac_extremes": (lambda: np.stack([stripes(1), stripes(0), pixel_checkerboard()]), 100, dict(
        ac_cat_max=10, no_eob=[0, 0, 4], eob_only=[2, 2, 2])),
    "long_runs_q75": (long_runs, 75, dict(zrl_max=3, zrl=18, no_eob=[4, 2], eob_only=[2, 4])),
    "long_runs_q50": (long_runs, 50, dict(zrl_max=3, zrl=18, no_eob=[4, 2], eob_only=[2, 4])),
    # seed 4: the first seed from 0 whose frame has blocks of all five shapes
    "writer_shapes": (lambda: single(writer_mix()), 100, dict(shapes=dict(a=45, b=3, c=5, d=16, e=1), raw_bytes=[1658])),
    "ends_mod4": (lambda: np.stack([noise_then_grey(s, 32) for s in ENDS]), 100, dict(
        raw_bytes=[408, 414, 403, 401, 412, 405, 394, 411], pad_bits=[0, 0, 0, 0, 6, 2, 6, 6])),
    "ends_1024": (lambda: single(noise_then_grey(10, 2496)), 100, dict(raw_bytes=[1024], pad_bits=[0])),
    "ends_1025": (lambda: single(noise_then_grey(17, 2528)), 100, dict(raw_bytes=[1025], pad_bits=[0])),
    "ends_2048": (lambda: single(noise_then_grey(10, 6592)), 100, dict(raw_bytes=[2048], pad_bits=[0])),
    # seeds 31 and 189: of the seeds below 4000 whose last byte padding completes to 0xFF, those where padding adds the fewest bits
    "last_ff_padded": (lambda: np.stack([np.random.default_rng(s).integers(0, 256, (8, 8, 3), dtype=np.uint8) for s in (31, 189)]), 100, dict(
        last_ff_by_padding=[True, True], raw_bytes=[238, 230], pad_bits=[4, 5])),
    # seed 394: the first seed from 0 of 0/255 grey noise whose two MCUs, behind ONE grey MCU, hold two 0xFF in a row that begin in lane 3 of a
    # word (at byte 319); 176 more grey MCUs (W = 16 * 179) move them to bytes 1023 and 1024.  Of 1500 seeds each of 0..255 and 0/255 noise none
    # held three in a row.
    "ff_placement": (lambda: single(grey_then_noise(394, 2864)), 100, dict(
        ff_at_1023=1, ff_at_0=1, ff_run_max=2, ff_lanes=[0, 1, 2, 3])),
    # seed 0: the first seed from 0 with ties of both signs in both tables
    "ties": (lambda: single(np.random.default_rng(0).integers(0, 256, (16, 16, 3), dtype=np.uint8)), 100, dict(
        ties_pos=[14, 10], ties_neg=[18, 5])),
    "colour_rounding": (lambda: single(colour_mcus()), 100, dict(eob_only=[1536])),
    "many_frames": (many_frames, 100, dict(frames=257)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(frames, quality, files, counters, expected figures) of one case: built and restated once, then left unchanged"""
    build, quality, expect = CASES[name]
    frames = np.ascontiguousarray(build())
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[-1] == 3
    frames.setflags(write=False)
    counters = {}
    files = tuple(jpeg_restated(frames, quality, counters))
    return frames, quality, files, counters, expect


def measured(counters):
    """the figures the cases are recorded by, from the restatement's counters of one call"""
    s = counters["streams"]
    ff = [i for one in s for i in one["ff_at"]]
    shapes = dict(a=0, b=0, c=0, d=0, e=0)
    for one in s:
        for k, v in writer_shapes(one).items():
            shapes[k] += int(v)
    return dict(
        frames=len(s),
        first_dc=[one["dc_diffs"][0][0] for one in s],
        dc11=[[sum(one["dc11_pos"][c] for one in s), sum(one["dc11_neg"][c] for one in s)] for c in range(2)],
        dc_cat_max=[max(n for one in s for n in range(12) if one["dc_cats"][c][n]) for c in range(2)],
        ac_cat_max=max(one["ac_cat_max"] for one in s),
        zrl=counters["zrl"], zrl_max=max(one["zrl_max"] for one in s),
        no_eob=[int(one["no_eob"]) for one in s], eob_only=[int(one["eob_only"]) for one in s],
        shapes=shapes,
        raw_bytes=[one["raw_bytes"] for one in s], pad_bits=[one["pad_bits"] for one in s],
        ff_at_1023=sum(i % 1024 == 1023 for i in ff), ff_at_0=sum(i % 1024 == 0 for i in ff),
        ff_lanes=sorted({i % 4 for i in ff}), ff_run_max=max([0] + [r for one in s for r in ff_runs(one)]),
        last_ff_by_padding=[one["last_ff_by_padding"] for one in s],
        ties_pos=counters["ties_pos"], ties_neg=counters["ties_neg"])


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_case_is_pillows_file(name):
    frames, quality, files, _, _ = case(name)
    for i, (f, ours) in enumerate(zip(frames, files)):
        theirs = pillow(f, quality)
        assert ours == theirs, (name, i, differ(ours, theirs))


@pytest.mark.parametrize("name", CASES)
def test_case_reaches_its_path(name):
    _, _, _, counters, expect = case(name)
    got = measured(counters)
    print(name, {k: got[k] for k in expect})
    for k, v in expect.items():
        assert got[k] == v, (name, k, got[k], v)


def test_the_paths_the_cases_exist_for():
    """what the recorded figures mean, said once more as conditions: were a figure in ``CASES`` re-recorded carelessly, this fails"""
    m = {name: measured(case(name)[3]) for name in CASES}
    assert m["dc_extremes"]["first_dc"][:2] == [-1024, 1016]                  # a black and a white first block
    assert min(m["dc_extremes"]["dc11"][0] + m["dc_extremes"]["dc11"][1]) > 0   # category 11, both signs, luma and chroma
    s = case("dc_extremes")[3]["streams"]
    assert {-2040, 2040, 0} <= set(s[0]["dc_diffs"][0][1:]) and {-2040, 2040} <= set(s[2]["dc_diffs"][1])
    assert m["ac_extremes"]["ac_cat_max"] == 10
    for name in ("long_runs_q75", "long_runs_q50"):
        assert m[name]["zrl_max"] == 3 and m[name]["no_eob"] == [4, 2] and m[name]["eob_only"] == [2, 4]
        blocks = case(name)[3]["streams"][1]["block_bits"]
        assert blocks[0] > blocks[1] == blocks[3] and blocks[2] > blocks[3]   # EOB-only blocks between long ones
    assert min(m["writer_shapes"]["shapes"].values()) > 0
    assert sorted(r % 4 for r in m["ends_mod4"]["raw_bytes"][:4]) == [0, 1, 2, 3] == sorted(r % 4 for r in m["ends_mod4"]["raw_bytes"][4:])
    assert m["ends_mod4"]["pad_bits"][:4] == [0] * 4 and min(m["ends_mod4"]["pad_bits"][4:]) > 0
    assert (m["ends_1024"]["raw_bytes"], m["ends_1025"]["raw_bytes"], m["ends_2048"]["raw_bytes"]) == ([1024], [1025], [2048])
    assert m["last_ff_padded"]["last_ff_by_padding"] == [True, True]
    p = m["ff_placement"]
    assert p["ff_at_1023"] and p["ff_at_0"] and p["ff_lanes"] == [0, 1, 2, 3] and p["ff_run_max"] >= 2
    ff = case("ff_placement")[3]["streams"][0]["ff_at"]
    assert any(i % 1024 == 1023 and i + 1 in ff for i in ff)                 # the two lie side by side across the chunks
    assert min(m["ties"]["ties_pos"] + m["ties"]["ties_neg"]) > 0
    assert m["many_frames"]["frames"] > 256 and len({len(f) for f in case("many_frames")[2]}) > 1


def test_dense_block_and_basis_block():
    zz, _ = T.blocks_restated(pixel_checkerboard(), J.lower_jpeg(16, 16, 100)["divisors"])
    assert zz[0, 0, 63] == -838 and np.count_nonzero(zz[0, 0]) == 17
    zz, _ = T.blocks_restated(stripes(1), J.lower_jpeg(16, 16, 100)["divisors"])
    assert zz[0, 0].min() == -924
    for q in (75, 50):
        zz, _ = T.blocks_restated(long_runs()[0], J.lower_jpeg(16, 16, q)["divisors"])
        assert (np.count_nonzero(zz[0, :4], axis=1) == 1).all() and (zz[0, :4, 63] != 0).all()


def test_colours_at_the_rounding_boundaries():
    colours = boundary_colours()
    assert colours.shape == (256, 3) and len({tuple(c) for c in colours.tolist()}) == 256
    assert {tuple(c) for c in colours[:8].tolist()} == {(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)}
    zz, _ = T.blocks_restated(colour_mcus(), J.lower_jpeg(256, 256, 100)["divisors"])
    assert not zz[:, :, 1:].any()
    near = np.zeros((3, 2), dtype=np.int64)
    for i, (r, g, b) in enumerate(colours.tolist()):
        # the conversion in exact arithmetic: Y to the nearest, half up; Cb and Cr to the nearest, half DOWN (libjpeg adds 32767, not 32768)
        y2 = 19595 * r + 38470 * g + 7471 * b
        cb2, cr2 = -11059 * r - 21709 * g + 32768 * b, 32768 * r - 27439 * g - 5329 * b
        # a flat block's only coefficient is its DC, 8 times the level at quality 100; chroma's 128 cancels against the level shift
        want = (8 * ((2 * y2 + 65536) // 131072 - 128), -8 * ((-2 * cb2 + 65536) // 131072), -8 * ((-2 * cr2 + 65536) // 131072))
        got = (int(zz[i, 0, 0]), int(zz[i, 4, 0]), int(zz[i, 5, 0]))
        assert got == want and (zz[i, :4, 0] == got[0]).all(), ("colour", (r, g, b), got, want)
        frac = [(y2 + 32768) & 0xFFFF, (cb2 + 32767) & 0xFFFF, (cr2 + 32767) & 0xFFFF]
        near += [[f <= 256, f >= 0xFFFF - 256] for f in frac]
    assert near.min() >= 41                                      # 248 colours dealt from six lists: 41 at least of each sum and side, within 256 / 65536


def test_no_stream_holds_four_ff_in_a_row():
    """Four 0xFF in a row are 32 1-bits.  No code is all 1-bits, so a run of 1-bits is at most the end of one code, the whole value
    behind it (category bits, all 1 for 2^n - 1) and the start of the next code; padding adds at most 7 behind a value."""
    huff = J.huffman_codes()
    codes = [(t, sy, int(huff[t, sy]) >> 16, int(huff[t, sy]) & 0xFFFF) for t in range(4) for sy in range(256) if huff[t, sy]]
    assert all(code != (1 << size) - 1 for _, _, size, code in codes)

    def ones(code, size, bits):                                  # 1-bits at the start or the end
        n = 0
        for i in bits(size):
            if not code >> i & 1:
                break
            n += 1
        return n

    lead = max(ones(code, size, lambda s: range(s - 1, -1, -1)) for _, _, size, code in codes)
    longest = max(ones(code, size, range) + min(sy if t in (0, 2) else sy & 15, 11 if t in (0, 2) else 10) + lead for t, sy, size, code in codes)
    assert lead == 15 and longest == 31 < 32


# ---- the mutation check ------------------------------------------------------------------------------------------------------------
# fault -> (the case that must catch it, where it changes a file by the counters)
FAULTS = {
    "one_zrl_per_gap": ("long_runs_q75", lambda m, c: m["zrl_max"] >= 2),
    "eob_always": ("ac_extremes", lambda m, c: sum(m["no_eob"]) > 0),
    "dc_category_clamped_at_10": ("dc_extremes", lambda m, c: max(m["dc_cat_max"]) == 11),
    "stuffing_dropped_at_chunk_end": ("ff_placement", lambda m, c: m["ff_at_1023"] > 0),
    "no_padding_in_a_last_word_of_one_byte": ("ends_mod4", lambda m, c: any(r % 4 == 1 and p for r, p in zip(m["raw_bytes"], m["pad_bits"]))),
    "negative_ties_toward_zero": ("ties", lambda m, c: sum(m["ties_neg"]) > 0),
    "file_offsets_restart_at_256": ("many_frames", lambda m, c: m["frames"] > 256),
}


def faulty_stream(zz, fault):
    """``stream_restated`` once more, without its counters, with one device mistake switched on"""
    huff = J.huffman_codes()
    acc, nacc, raw = 0, 0, bytearray()

    def put(table, symbol, extra=0, nextra=0):
        nonlocal acc, nacc
        size, code = int(huff[table, symbol]) >> 16, int(huff[table, symbol]) & 0xFFFF
        acc = ((acc << size | code) << nextra) | extra
        nacc += size + nextra
        whole = nacc // 8
        raw.extend((acc >> (nacc - 8 * whole)).to_bytes(whole, "big"))
        nacc -= 8 * whole
        acc &= (1 << nacc) - 1

    def magnitude(v, most):
        n = min(int(abs(v)).bit_length(), most)
        return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)

    pred = [0, 0, 0]
    for mcu in zz:
        for j, blk in enumerate(mcu):
            comp = max(j - 3, 0)
            dc, ac = (0, 1) if comp == 0 else (2, 3)
            n, bits = magnitude(int(blk[0]) - pred[comp], 10 if fault == "dc_category_clamped_at_10" else 11)
            pred[comp] = int(blk[0])
            put(dc, n, bits, n)
            last = 0
            for k in np.nonzero(blk[1:])[0] + 1:
                run = int(k) - last - 1
                if run > 15 and fault == "one_zrl_per_gap":
                    put(ac, 0xF0)
                    run = (run - 16) % 16
                while run > 15:
                    put(ac, 0xF0)
                    run -= 16
                n, bits = magnitude(int(blk[k]), 10)
                put(ac, run << 4 | n, bits, n)
                last = int(k)
            if last < 63 or fault == "eob_always":
                put(ac, 0)
    pad = -nacc % 8
    if pad:
        skip = fault == "no_padding_in_a_last_word_of_one_byte" and len(raw) % 4 == 0
        raw.append((acc << pad) | (0 if skip else (1 << pad) - 1))
    out = bytearray()
    for i, b in enumerate(raw):
        out.append(b)
        if b == 0xFF and not (fault == "stuffing_dropped_at_chunk_end" and i % 1024 == 1023):
            out.append(0)
    return bytes(out)


def faulty_files(frames, quality, fault=None):
    """``jpeg_restated`` once more with ``fault``; with None it must be the restatement"""
    H, W = frames.shape[-3:-1]
    low = J.lower_jpeg(H, W, quality)
    files = []
    for f in frames:
        zz, dummy = T.blocks_restated(f, low["divisors"])
        if fault == "negative_ties_toward_zero":                 # floor instead of truncate: -2.5 becomes -2
            my, mx = (H + 15) // 16, (W + 15) // 16
            y, cb, cr = T.planes_restated(f)
            yb = y.reshape(my, 2, 8, mx, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my * mx, 4, 8, 8)
            cbb, crb = (c.reshape(my, 8, mx, 8).transpose(0, 2, 1, 3).reshape(my * mx, 1, 8, 8) for c in (cb, cr))
            coef = T.fdct_islow(np.concatenate([yb, cbb, crb], axis=1) - 128).reshape(my * mx, 6, 64)
            div = np.asarray(low["divisors"], dtype=np.int64)[[0, 0, 0, 0, 1, 1]][None]
            tie = ((coef < 0) & ((np.abs(coef) + (div >> 1)) % div == 0) & ~dummy[:, :, None])[:, :, J.ZIGZAG]
            zz = zz + tie
            for j in range(1, 4):
                zz[dummy[:, j], j, 0] = zz[dummy[:, j], j - 1, 0]
        files.append(low["header"] + faulty_stream(zz, fault) + b"\xff\xd9")
    if fault == "file_offsets_restart_at_256":                   # the scan's carry is lost between its passes of 256
        at = [0]
        for i, f in enumerate(files):
            at.append((0 if i > 0 and i % 256 == 0 else at[-1]) + len(f))
        buf = bytearray(sum(len(f) for f in files))
        for i, f in enumerate(files):
            buf[at[i]:at[i] + len(f)] = f
        files = [bytes(buf[at[i]:at[i + 1]]) for i in range(len(files))]
    return files


def small(name):
    frames = case(name)[0]
    return frames.shape[0] * math.ceil(frames.shape[1] / 16) * math.ceil(frames.shape[2] / 16) <= 64


def test_the_copy_without_a_fault_is_the_restatement():
    for name in CASES:
        if small(name) or name == "ff_placement":
            frames, quality, files, _, _ = case(name)
            assert tuple(faulty_files(frames, quality)) == files, name


@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_is_caught_by_its_case(fault):
    named, trigger = FAULTS[fault]
    caught = []
    for name in CASES:
        frames, quality, files, counters, _ = case(name)
        expected = bool(trigger(measured(counters), counters))
        if not (expected or small(name)):
            continue                                             # (a large case that the counters say is untouched: not run)
        differs = tuple(faulty_files(frames, quality, fault)) != files
        assert differs == expected, (fault, name, differs, expected)
        caught += [name] if differs else []
    print(fault, "caught by", caught)
    assert named in caught


# the faults that tests/test_jpeg_host.py's SHAPES x CONTENTS do not trigger, by the same counters: at all of its QUALITIES, on the host, and
# at the qualities tests/test_gpu_jpeg.py runs them with on the device (100 and 30; 95 and 1 too at 17 x 23)
MISSED_BY_THE_OLD_CASES = ("file_offsets_restart_at_256",)
MISSED_BY_THE_OLD_DEVICE_CASES = ("file_offsets_restart_at_256",)


def test_faults_the_old_cases_missed():
    hit, hit_device = set(), set()
    for H, W in T.SHAPES:
        for kind in T.CONTENTS:
            for q in T.QUALITIES:
                c = {}
                jpeg_restated(T.content(kind, H, W), q, c)
                m = measured(c)
                now = {fault for fault, (_, trigger) in FAULTS.items() if trigger(m, c)}
                hit |= now
                hit_device |= now if q in (100, 30) or (H, W) == (17, 23) and q in (95, 1) else set()
    missed, missed_device = (tuple(f for f in FAULTS if f not in h) for h in (hit, hit_device))
    print("the old cases miss:", missed, "and on the device:", missed_device)
    assert missed == MISSED_BY_THE_OLD_CASES and missed_device == MISSED_BY_THE_OLD_DEVICE_CASES
