"""Host side of the JPEG encoder (3d-magic-mirror_amd/jpeg.py, csrc/mm_jpeg.hip), no GPU.

This file holds the RESTATEMENT: libjpeg's baseline path in plain numpy integer arithmetic, in the order DESIGN.md states -- colour
conversion, edge replication, h2v2 downsampling with the alternating bias, the islow forward DCT, quantisation rounding half away from
zero, dummy blocks, the interleaved scan with the standard Huffman tables, padding with 1-bits and 0xFF stuffing -- on whole images.
tests/test_gpu_jpeg.py holds the device to it byte for byte.  Here the restatement is held to live Pillow the same way: the COMPLETE file
that ``Image.fromarray(f).save(buf, 'JPEG', quality=q)`` writes, with no tolerance, because nothing on either side is rounded in floating
point.  The restatement counts what it emits (ZRL codes, stuffed bytes, padding bits, dummy blocks), and the tests assert on those
counters that the cases reach every path.  Only the tests that compare with Pillow need it: the restatement, its counters, the tables,
the argument and ABI tests run without it, and so does tests/test_gpu_jpeg.py, which imports the restatement from here.

The inputs here (noise, ramps, flat frames, renders) reach the entropy coder's discrete paths by chance.  tests/test_jpeg_edges_host.py builds an
input for each path and asserts it from the per-stream records that ``stream_restated`` keeps (``stream_counters``, ``writer_shapes``,
``ff_runs``) and the ties that ``blocks_restated`` counts; tests/test_gpu_jpeg_edges.py runs those inputs on the device."""
import importlib
import io

import numpy as np
import pytest
import torch

J = importlib.import_module("3d-magic-mirror_amd.jpeg")
S = importlib.import_module("3d-magic-mirror_amd.synthetic")

SHAPES = ((1, 1), (8, 8), (16, 16), (17, 23), (24, 40), (40, 24), (33, 9), (50, 70), (128, 64))
CONTENTS = ("noise", "ramp", "black", "white", "binary", "render")
QUALITIES = (100, 95, 75, 30, 1)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def fdct_islow(d):
    """jfdctint on (...,8,8) int64 samples minus 128: rows first, then columns; the output is scaled by 8"""
    C, P = 13, 2

    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    def one_pass(v, first):                                     # along the last axis
        d0, d1, d2, d3, d4, d5, d6, d7 = (v[..., i] for i in range(8))
        t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        n = C - P if first else C + P
        o0 = (t10 + t11) << P if first else descale(t10 + t11, P)
        o4 = (t10 - t11) << P if first else descale(t10 - t11, P)
        z1 = (t12 + t13) * 4433
        o2 = descale(z1 + t13 * 6270, n)
        o6 = descale(z1 + t12 * -15137, n)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * 9633
        t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        return np.stack([o0, descale(t7 + z1 + z4, n), o2, descale(t6 + z2 + z3, n), o4, descale(t5 + z2 + z4, n), o6,
                         descale(t4 + z1 + z3, n)], axis=-1)

    rows = one_pass(d.astype(np.int64), True)
    return np.swapaxes(one_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def planes_restated(f):
    """(Y, Cb, Cr) of one (H,W,3) uint8 frame, padded to whole MCUs: Y (16my,16mx), Cb and Cr (8my,8mx), int64"""
    H, W = f.shape[:2]
    my, mx = (H + 15) // 16, (W + 15) // 16
    r, g, b = (f[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    # columns: the input's last column up to the MCU; rows: the input's last row up to an even height
    rows, cols = np.minimum(np.arange(H + H % 2), H - 1), np.minimum(np.arange(16 * mx), W - 1)
    out = [y[np.minimum(np.arange(16 * my), H - 1)][:, cols]]
    bias = np.tile(np.array([1, 2], dtype=np.int64), 4 * mx)
    for c in (cb, cr):
        c = c[rows][:, cols]
        c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        out.append(c[np.minimum(np.arange(8 * my), c.shape[0] - 1)])          # the DOWNSAMPLED last row up to the MCU
    return out


def blocks_restated(f, divisors, counters=None):
    """(mcus,6,64) quantised coefficients in zigzag order, MCU order, and (mcus,6) bool: which blocks are dummies.
    counters, if given: ties_pos and ties_neg, [luma, chroma], the coefficients of real blocks that lie exactly half way (they round away from zero)"""
    H, W = f.shape[:2]
    my, mx = (H + 15) // 16, (W + 15) // 16
    y, cb, cr = planes_restated(f)
    yb = y.reshape(my, 2, 8, mx, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my * mx, 4, 8, 8)
    cbb, crb = (c.reshape(my, 8, mx, 8).transpose(0, 2, 1, 3).reshape(my * mx, 1, 8, 8) for c in (cb, cr))
    coef = fdct_islow(np.concatenate([yb, cbb, crb], axis=1) - 128).reshape(my * mx, 6, 64)
    div = np.asarray(divisors, dtype=np.int64)[[0, 0, 0, 0, 1, 1]][None]
    q = np.sign(coef) * ((np.abs(coef) + (div >> 1)) // div)                                     # half away from zero
    m = np.arange(my * mx)
    by, bx = 2 * (m // mx)[:, None] + np.array([0, 0, 1, 1]), 2 * (m % mx)[:, None] + np.array([0, 1, 0, 1])
    dummy = np.concatenate([(by >= (H + 7) // 8) | (bx >= (W + 7) // 8), np.zeros((my * mx, 2), dtype=bool)], axis=1)
    if counters is not None:
        tie = ((np.abs(coef) + (div >> 1)) % div == 0) & ~dummy[:, :, None]
        for key, sign in (("ties_pos", coef > 0), ("ties_neg", coef < 0)):
            counters.setdefault(key, [0, 0])
            counters[key][0] += int((tie & sign)[:, :4].sum())
            counters[key][1] += int((tie & sign)[:, 4:].sum())
    for j in range(1, 4):                                        # a dummy block: no AC, the DC of the block before it in MCU order
        q[dummy[:, j], j, :] = 0
        q[dummy[:, j], j, 0] = q[dummy[:, j], j - 1, 0]
    return q[:, :, J.ZIGZAG], dummy


def stream_restated(zz, counters):
    """the entropy-coded bytes of (mcus,6,64) zigzag coefficients: interleaved Y00 Y01 Y10 Y11 Cb Cr, one DC predictor per component.
    What it emitted goes into counters: the sums zrl and stuffed, pad_bits of this stream, and one dict per stream appended to
    counters["streams"] (see ``stream_counters``).  The counters observe; nothing below reads them."""
    huff = J.huffman_codes()
    seen = stream_counters()
    acc, nacc, raw = 0, 0, bytearray()                           # the bits not yet in raw: fewer than 8 between two symbols

    def put(table, symbol, extra=0, nextra=0):
        nonlocal acc, nacc
        size, code = int(huff[table, symbol]) >> 16, int(huff[table, symbol]) & 0xFFFF
        assert size > 0
        acc = ((acc << size | code) << nextra) | extra
        nacc += size + nextra
        whole = nacc // 8
        raw.extend((acc >> (nacc - 8 * whole)).to_bytes(whole, "big"))
        nacc -= 8 * whole
        acc &= (1 << nacc) - 1

    def magnitude(v):
        n = int(abs(v)).bit_length()
        return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)

    pred = [0, 0, 0]
    for mcu in zz:
        for j, blk in enumerate(mcu):
            comp = max(j - 3, 0)
            dc, ac = (0, 1) if comp == 0 else (2, 3)
            seen["block_at"].append(8 * len(raw) + nacc)
            diff = int(blk[0]) - pred[comp]
            n, bits = magnitude(diff)
            seen["dc_diffs"][min(comp, 1)].append(diff)
            seen["dc_cats"][min(comp, 1)][n] += 1
            if n == 11:
                seen["dc11_pos" if diff > 0 else "dc11_neg"][min(comp, 1)] += 1
            pred[comp] = int(blk[0])
            put(dc, n, bits, n)
            last = 0
            for k in np.nonzero(blk[1:])[0] + 1:
                run = int(k) - last - 1
                zrls = 0
                while run > 15:
                    put(ac, 0xF0)
                    counters["zrl"] += 1
                    zrls += 1
                    run -= 16
                n, bits = magnitude(int(blk[k]))
                seen["zrl_max"], seen["ac_cat_max"] = max(seen["zrl_max"], zrls), max(seen["ac_cat_max"], n)
                put(ac, run << 4 | n, bits, n)
                last = int(k)
            if last < 63:
                put(ac, 0)
            seen["no_eob"] += last == 63
            seen["eob_only"] += last == 0
            seen["block_bits"].append(8 * len(raw) + nacc - seen["block_at"][-1])
    pad = -nacc % 8                                              # the last byte is filled with 1-bits
    counters["pad_bits"] = pad
    if pad:
        raw.append((acc << pad) | ((1 << pad) - 1))
    counters["stuffed"] += raw.count(b"\xff")
    seen["pad_bits"], seen["raw_bytes"] = pad, len(raw)
    seen["ff_at"] = [i for i, b in enumerate(raw) if b == 0xFF]
    seen["last_ff"] = raw[-1] == 0xFF
    seen["last_ff_by_padding"] = bool(pad) and raw[-1] == 0xFF     # the stuffed 0x00 then comes just before EOI
    counters.setdefault("streams", []).append(seen)
    return bytes(raw).replace(b"\xff", b"\xff\x00")


def stream_counters():
    """what ``stream_restated`` records of one stream; [luma, chroma] where a figure is kept per component class"""
    return dict(dc_cats=[[0] * 12, [0] * 12],                    # how many DC differences of each category 0..11
                dc11_pos=[0, 0], dc11_neg=[0, 0],                # the signs of the differences of category 11
                dc_diffs=[[], []],                               # every DC difference, in coding order
                ac_cat_max=0,                                    # the largest AC category
                zrl_max=0,                                       # the most ZRLs before one coefficient
                no_eob=0, eob_only=0,                            # blocks whose coefficient 63 is non-zero; blocks with no AC at all
                block_at=[], block_bits=[],                      # every block's bit offset in the stream and its bit length
                pad_bits=0, raw_bytes=0,                         # the stream before stuffing, padding included
                ff_at=[],                                        # the index of every 0xFF in it
                last_ff=False, last_ff_by_padding=False)


def writer_shapes(seen):
    """how many blocks of one stream take each way through the device's JpegWriter, which ORs a block's bits into big-endian 32-bit
    words: the first word it flushes and the word ``finish`` completes are shared with the neighbours (atomic OR), the words between
    are stored plainly.  a: begins and ends inside one word (no flush); b: begins inside a word and ends exactly at its end (the flush
    is the OR, ``finish`` has nothing left); c: begins at bit 0 of a word; d: touches three words or more (plain stores between the
    ORs); e: ends exactly on a word boundary after a plain store.  A block can have several."""
    out = dict(a=0, b=0, c=0, d=0, e=0)
    for at, n in zip(seen["block_at"], seen["block_bits"]):
        s = at % 32
        out["a"] += s + n < 32
        out["b"] += s > 0 and s + n == 32
        out["c"] += s == 0
        out["d"] += (at + n - 1) // 32 - at // 32 >= 2
        out["e"] += s + n >= 64 and (s + n) % 32 == 0
    return out


def ff_runs(seen):
    """the lengths of the runs of consecutive 0xFF in a stream before stuffing, in order"""
    runs, prev = [], None
    for i in seen["ff_at"]:
        if prev is not None and i == prev + 1:
            runs[-1] += 1
        else:
            runs.append(1)
        prev = i
    return runs


def jpeg_restated(frames, quality=100, counters=None):
    """the files of (...,H,W,3) uint8 frames (a torch tensor or an array, on the host) as a list of bytes, in row-major order"""
    f = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    assert f.dtype == np.uint8 and f.shape[-1] == 3
    H, W = f.shape[-3:-1]
    low = J.lower_jpeg(H, W, quality)
    counters = counters if counters is not None else {}
    for key in ("zrl", "stuffed", "pad_bits", "dummy_right", "dummy_below"):
        counters.setdefault(key, 0)
    files = []
    for one in f.reshape(-1, H, W, 3):
        zz, dummy = blocks_restated(one, low["divisors"], counters)
        counters["dummy_right"] += int(dummy[:, 1].sum())
        counters["dummy_below"] += int(dummy[:, 2].sum())
        files.append(low["header"] + stream_restated(zz, counters) + b"\xff\xd9")
    return files


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def content(kind, H, W, seed=0):
    """(H,W,3) uint8"""
    g = np.random.default_rng(1000 * H + W + seed)
    if kind == "noise":
        return g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([(255 * x) // max(W - 1, 1), (255 * y) // max(H - 1, 1), (255 * (x + y)) // max(H + W - 2, 1)], axis=-1).astype(np.uint8)
    if kind in ("black", "white"):
        return np.full((H, W, 3), 0 if kind == "black" else 255, dtype=np.uint8)
    if kind == "binary":
        return (g.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    assert kind == "render"                                      # synthetic's ground truth: texture inside its silhouette, over white
    gt = S.synthetic_batch(torch.zeros(4, 3), 1, H, W, seed=H + W + seed)[1][0]
    return (gt[:3] * gt[3:] + (1 - gt[3:])).mul(255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def pil_image():
    """live Pillow, for the tests that compare with it; they alone skip where it does not import"""
    return pytest.importorskip("PIL.Image")


def pillow(f, quality):
    buf = io.BytesIO()
    Image = pil_image()
    Image.fromarray(f).save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def differ(a, b):
    """where two files part, for the message"""
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return "%d and %d bytes, first difference at %d" % (len(a), len(b), n)


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_restatement_is_pillows_file(H, W):
    for kind in CONTENTS:
        f = content(kind, H, W)
        for q in QUALITIES:
            ours, = jpeg_restated(f, q)
            theirs = pillow(f, q)
            assert ours == theirs, (kind, q, differ(ours, theirs))


def test_every_quality_on_one_image():
    f = content("noise", 16, 16, seed=3)
    for q in range(1, 101):
        ours, = jpeg_restated(f, q)
        assert ours == pillow(f, q), q


def test_cases_reach_every_path():
    total = {}
    aligned = 0
    for H, W in SHAPES:
        for kind in CONTENTS:
            for q in QUALITIES:
                c = {}
                jpeg_restated(content(kind, H, W), q, c)
                aligned += c["pad_bits"] == 0
                for k, v in c.items():
                    if isinstance(v, int):                       # (the sums; the per-stream records are tests/test_jpeg_edges_host.py's)
                        total[k] = total.get(k, 0) + v
    assert total["zrl"] > 0                                      # runs of 16 zeros
    assert total["stuffed"] > 0                                  # a 0xFF in the stream
    assert aligned > 0                                           # a stream that ends on a byte boundary: no padding
    c = {}
    jpeg_restated(content("noise", 17, 23), 100, c)
    assert c["dummy_right"] > 0 and c["dummy_below"] > 0         # dummies in both directions in one frame
    c = {}
    jpeg_restated(content("black", 16, 16), 100, c)
    assert c["dummy_right"] == 0 and c["dummy_below"] == 0


def test_flat_frames_code_to_a_few_bytes():
    low = J.lower_jpeg(50, 70, 100)
    for kind in ("black", "white"):
        c = {}
        ours, = jpeg_restated(content(kind, 50, 70), 100, c)
        # every block is "difference 0, EOB", 6 bits at most (2 + 4 luma, 2 + 2 chroma), but each component's first: a DC of 20 bits at most
        assert len(ours) - len(low["header"]) - 2 - c["stuffed"] <= (low["blocks"] * 6 + 3 * 20 + 7) // 8


def test_header_is_pillows():
    for (H, W), q in (((1, 1), 100), ((17, 23), 75), ((128, 64), 100), ((300, 260), 30)):
        low = J.lower_jpeg(H, W, q)
        theirs = pillow(np.zeros((H, W, 3), dtype=np.uint8), q)
        head = low["header"]
        assert theirs[:len(head)] == head


def test_header_segments_and_params_layout():
    for (H, W), q in (((1, 1), 100), ((17, 23), 75), ((300, 260), 30)):
        low = J.lower_jpeg(H, W, q)
        head = low["header"]
        assert head[:2] == b"\xff\xd8" and head[2:4] == b"\xff\xe0" and head[6:11] == b"JFIF\0" and head[-14:-12] == b"\xff\xda"
        assert head.count(b"\xff\xdb\x00\x43") == 2 and head.count(b"\xff\xc4") == 4
        sof = head.index(b"\xff\xc0")
        assert head[sof + 5:sof + 9] == H.to_bytes(2, "big") + W.to_bytes(2, "big")
        assert low["params"].dtype == torch.int32 and low["params"].numel() == 128 + 1024 + (len(head) + 3) // 4
        assert np.array_equal(low["params"][:128].numpy().reshape(2, 64), low["divisors"])
        assert np.array_equal(low["params"][128:128 + 1024].numpy().reshape(4, 256), J.huffman_codes())
        assert bytes(low["params"][128 + 1024:].numpy().view(np.uint8)[:len(head)]) == head


def test_quant_tables_match_for_every_quality():
    f = np.zeros((8, 8, 3), dtype=np.uint8)
    Image = pil_image()
    for q in range(1, 101):
        with Image.open(io.BytesIO(pillow(f, q))) as im:
            theirs = im.quantization
        ours = J.quant_tables(q)
        for t in range(2):
            got = list(theirs[t])
            # Pillow hands tables over in zigzag or in natural order, by version: one of the two must be ours
            assert got == [int(v) for v in ours[t][J.ZIGZAG]] or got == [int(v) for v in ours[t]], q


def test_quality_scaling():
    for q in range(1, 101):
        ours = J.quant_tables(q)
        assert np.array_equal(J.lower_jpeg(8, 8, q)["divisors"], 8 * ours) and ours.min() >= 1 and ours.max() <= 255
    assert (J.quant_tables(100) == 1).all() and J.quant_tables(50)[0, 0] == 16 and J.quant_tables(50)[1, 0] == 17
    assert J.quant_tables(1).max() == 255 and J.quant_tables(25)[0, 0] == 32 and J.quant_tables(75)[0, 0] == 8


def test_bounds():
    low = J.lower_jpeg(256, 256, 100)
    assert (low["mcu_rows"], low["mcu_cols"], low["blocks"]) == (16, 16, 1536)
    assert low["stream_capacity"] >= 1536 * 208 and low["stream_capacity"] % 1024 == 0
    assert low["file_capacity"] == len(low["header"]) + 2 * low["stream_capacity"] + 2
    assert low["workspace_bytes"](3) >= 3 * (1536 * 128 + 1536 * 4 + low["stream_capacity"])
    assert low["files_offset"](3) == 256 and low["files_offset"](32) == 512
    # the worst a block codes to: DC category 11 behind an 11-bit code at most, 63 coefficients of category 10 behind 16-bit codes
    sizes = J.huffman_codes() >> 16
    assert int(sizes[[0, 2]].max()) + 11 + 63 * (int(sizes[[1, 3]].max()) + 10) <= 8 * J.BLOCK_BYTES
    ours, = jpeg_restated(content("binary", 128, 64), 100)
    assert len(ours) <= J.lower_jpeg(128, 64, 100)["file_capacity"]
    for H, W in ((0, 8), (8, 0), (65536, 8), (16384, 16384)):
        with pytest.raises(ValueError):
            J.lower_jpeg(H, W, 100)


def test_argument_errors(pkg):
    ok = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="export_images"):
        pkg.encode_jpeg(ok.float())
    with pytest.raises(ValueError, match="uint8"):
        pkg.encode_jpeg(ok.int())
    for bad in (torch.zeros((2, 8, 8, 4), dtype=torch.uint8), torch.zeros((2, 3, 8, 8), dtype=torch.uint8), torch.zeros((8, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="H,W,3"):
            pkg.encode_jpeg(bad)
    with pytest.raises(ValueError, match="empty"):
        pkg.encode_jpeg(ok[:0])
    for q in (0, 101, -1, 99.5, None, True):
        with pytest.raises(ValueError, match="quality"):
            pkg.encode_jpeg(ok, quality=q)
    with pytest.raises(RuntimeError, match="device"):            # a host tensor: there is no CPU fallback
        pkg.encode_jpeg(ok)
    assert pkg.lower_jpeg is J.lower_jpeg and pkg.JpegBatch is J.JpegBatch


def test_batch_indexing_and_write(tmp_path):
    frames = np.stack([content(k, 5, 7) for k in ("noise", "black", "ramp")])
    files = jpeg_restated(frames, 90)
    assert len({len(x) for x in files}) > 1
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in files])])
    batch = J.JpegBatch(torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy()), offsets)
    assert len(batch) == 3 and batch.shape == (3,) and list(batch) == files
    assert batch[-1] == files[2] and isinstance(batch[0], bytes)
    with pytest.raises(IndexError):
        batch[3]
    with pytest.raises(TypeError):
        batch[0:2]
    paths = [tmp_path / ("%d.jpg" % i) for i in range(3)]
    batch.write(paths)
    assert [p.read_bytes() for p in paths] == files
    with pytest.raises(ValueError):
        batch.write(paths[:2])


def test_files_open_in_pillow():
    Image = pil_image()
    for i, data in enumerate(jpeg_restated(np.stack([content(k, 5, 7) for k in ("noise", "black", "ramp")]), 90)):
        with Image.open(io.BytesIO(data)) as im:
            assert im.size == (7, 5) and im.mode == "RGB" and im.format == "JPEG", i
            im.load()


def test_abi_mirror_and_return_codes():
    import ctypes
    N = importlib.import_module("3d-magic-mirror_amd._native")
    L = N.lib()
    assert L.mm_abi_version() == 9 == N.ABI_VERSION
    assert L.mm_struct_size(37) == ctypes.sizeof(N.MMJpegDesc) > 0
    assert {"mm_jpeg_query_workspace", "mm_jpeg_files_offset", "mm_jpeg_encode"} <= set(N.EXPORTS)
    low = J.lower_jpeg(17, 23, 75)
    par = low["params"].numpy().copy()
    keep = ctypes.create_string_buffer(64)
    fake = ctypes.c_void_p(ctypes.addressof(keep) + 15 & ~15)    # never dereferenced: every refusal comes before any GPU work

    def desc(n=3, H=17, W=23, params=par):
        d = N.MMJpegDesc()
        d.n, d.H, d.W, d.header_bytes = n, H, W, len(low["header"])
        d.frames = d.params = d.workspace = fake
        d.params_host = ctypes.c_void_p(params.ctypes.data)
        d.workspace_bytes = L.mm_jpeg_query_workspace(ctypes.byref(d))
        return d

    d = desc()
    for n in (1, 3, 48):                                         # lower_jpeg's bounds are the library's
        d.n = n
        assert L.mm_jpeg_query_workspace(ctypes.byref(d)) == low["workspace_bytes"](n) > n * low["file_capacity"]
        assert L.mm_jpeg_files_offset(ctypes.byref(d)) == low["files_offset"](n)
    assert L.mm_jpeg_encode(None, None) == -1
    d = desc()
    d.frames = None
    assert L.mm_jpeg_encode(ctypes.byref(d), None) == -1
    for kw in (dict(n=0), dict(H=0), dict(W=-1)):
        d = desc(**kw)
        assert L.mm_jpeg_encode(ctypes.byref(d), None) == -2 and d.workspace_bytes == 0, kw
    for kw in (dict(H=65536), dict(n=65536), dict(H=16384, W=16384)):
        d = desc(**kw)
        assert L.mm_jpeg_encode(ctypes.byref(d), None) == -5 and d.workspace_bytes == 0, kw
    d = desc()
    d.header_bytes = 1
    assert L.mm_jpeg_encode(ctypes.byref(d), None) == -2
    d = desc()
    d.workspace_bytes -= 1
    assert L.mm_jpeg_encode(ctypes.byref(d), None) == -3
    d = desc()
    d.workspace = ctypes.c_void_p(fake.value + 4)
    assert L.mm_jpeg_encode(ctypes.byref(d), None) == -3
    for word, value in ((0, 0), (5, 12), (127, 8 * 256), (128 + 0, 17 << 16), (128 + 1, 2 << 16 | 4)):
        bad = par.copy()                                         # a divisor that is not 8 * (1..255); a code of 17 bits; a code wider than its size
        bad[word] = value
        assert L.mm_jpeg_encode(ctypes.byref(desc(params=bad)), None) == -2, (word, value)
    bad = par.copy()
    bad[128 + 256 + 0x0B] = 16 << 16 | 1                         # 16 bits before 11 category bits: more than a block's room allows
    assert L.mm_jpeg_encode(ctypes.byref(desc(params=bad)), None) == -2
