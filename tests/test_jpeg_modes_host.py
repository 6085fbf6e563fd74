"""Host side of the JPEG layouts beyond 4:2:0 (3d-magic-mirror_amd/jpeg.py ``encode_jpeg`` / ``jpeg_roundtrip`` with ``mode`` and
``subsampling``, csrc/mm_jpeg.hip), no GPU.

This file holds the RESTATEMENT of libjpeg's encoder and decoder for greyscale, 4:4:4 and 4:2:2 in plain numpy integer arithmetic, built
from the pieces of tests/test_jpeg_host.py (``fdct_islow``) and tests/test_jpeg_roundtrip_host.py (``samples_restated``, ``natural``): what
an MCU is, how edges replicate, h2v1 downsampling with its alternating bias, dummy Y1 blocks, the scan's block order and predictors, and
for the decoder h2v1 "fancy" upsampling or replication and no upsampling at all.  It is held to live Pillow with no tolerance: the COMPLETE
file ``Image.fromarray(f).save(buf, 'JPEG', quality=q, subsampling=s)`` writes, and the whole array ``Image.open`` gives back.  Where the
written rules and Pillow disagree, Pillow wins.  tests/test_gpu_jpeg_modes.py holds the device to the restatement (and to Pillow).

The restatement counts what it reaches and the tests assert on those counters; a copy of it with six switchable faults shows that the
cases catch each of them: the yardstick can fail.  Only the tests that compare with Pillow need it."""
import functools
import importlib
import io

import numpy as np
import pytest
import torch

from test_jpeg_host import CONTENTS, content, differ, fdct_islow, jpeg_restated, pil_image
from test_jpeg_roundtrip_host import grey_content, natural, new_counters, samples_restated

J = importlib.import_module("3d-magic-mirror_amd.jpeg")

LAYOUTS = ("L", "4:4:4", "4:2:2")
SHAPES = ((1, 1), (8, 8), (7, 9), (9, 7), (16, 16), (17, 23), (24, 40), (33, 9), (1, 40), (40, 1), (128, 64))
# 4:2:2 decoding: W of 2..6 around the narrow-chroma rule (fancy upsampling begins at three chroma columns, W = 5), and odd sizes
DECODE_422_SHAPES = SHAPES + ((3, 2), (3, 3), (3, 4), (3, 5), (3, 6), (5, 7), (31, 18))
GREY_CONTENTS = ("noise", "mask", "blob", "ramp", "black", "white")          # six masks: grey_content's four and the two flat ones
QUALITIES = (100, 30, 1)
FAULTS = ("bias_10", "dummy_own_coef", "grey_chroma_table", "y1_pred_prev_mcu", "h2v1_rounding_swapped", "fancy_when_narrow")
# the component of every block of an MCU
COMPONENTS = {"L": (0,), "4:4:4": (0, 1, 2), "4:2:2": (0, 0, 1, 2)}


# ---- the restatement: encoding ------------------------------------------------------------------------------------------------------
def frame_of(kind, H, W, layout):
    """(H,W) uint8 for layout "L", else (H,W,3)"""
    if layout != "L":
        return content(kind, H, W)
    if kind in ("black", "white"):
        return np.full((H, W), 0 if kind == "black" else 255, dtype=np.uint8)
    return grey_content(kind, H, W)


def contents_of(layout):
    return GREY_CONTENTS if layout == "L" else CONTENTS


def blocks_of(plane, by, bx):
    """(8 by, 8 bx) -> (by, bx, 8, 8)"""
    return plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3)


def mcus_restated(f, layout, divisors, faults=()):
    """(mcus, blocks per MCU, 64) quantised coefficients in zigzag order, MCU order, and (mcus, blocks per MCU) bool: the dummies"""
    H, W = f.shape[:2]
    low = J.lower_jpeg(H, W, 100, "L" if layout == "L" else "RGB", "4:2:0" if layout == "L" else layout)
    my, mx = low["mcu_rows"], low["mcu_cols"]
    assert (low["mcu_height"], low["mcu_width"], low["blocks_per_mcu"]) == {"L": (8, 8, 1), "4:4:4": (8, 8, 3), "4:2:2": (8, 16, 4)}[layout]
    rows = np.minimum(np.arange(8 * my), H - 1)                  # rows beyond H: the last row, up to the block
    cols = np.minimum(np.arange(low["mcu_width"] * mx), W - 1)   # columns beyond W: the input's last column, up to the MCU
    dummy = np.zeros((my * mx, low["blocks_per_mcu"]), dtype=bool)
    if layout == "L":
        planes = [f.astype(np.int64)]
    else:
        r, g, b = (f[..., c].astype(np.int64) for c in range(3))
        planes = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                  (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                  (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16]
    planes = [p[rows][:, cols] for p in planes]
    if layout == "4:2:2":
        bias = np.tile(np.array([1, 0] if "bias_10" in faults else [0, 1], dtype=np.int64), 4 * mx)
        y = blocks_of(planes[0], my, 2 * mx).reshape(my, mx, 2, 8, 8)
        chroma = [blocks_of((c[:, 0::2] + c[:, 1::2] + bias) >> 1, my, mx)[:, :, None] for c in planes[1:]]
        blocks = np.concatenate([y] + chroma, axis=2)
        dummy[:, 1] = 2 * (np.arange(my * mx) % mx) + 1 >= (W + 7) // 8
    else:
        blocks = np.stack([blocks_of(p, my, mx) for p in planes], axis=2)
    coef = fdct_islow(blocks.reshape(my * mx, -1, 8, 8) - 128).reshape(my * mx, -1, 64)
    tables = [1 if c else 0 for c in COMPONENTS[layout]]
    if layout == "L" and "grey_chroma_table" in faults:
        tables = [1]
    div = np.asarray(divisors, dtype=np.int64)[tables][None]
    q = np.sign(coef) * ((np.abs(coef) + (div >> 1)) // div)    # half away from zero
    if layout == "4:2:2" and "dummy_own_coef" not in faults:    # a dummy: no AC, Y0's DC
        q[dummy[:, 1], 1, :] = 0
        q[dummy[:, 1], 1, 0] = q[dummy[:, 1], 0, 0]
    return q[:, :, J.ZIGZAG], dummy


def stream_of(zz, layout, counters, faults=()):
    """the entropy-coded bytes of (mcus, blocks per MCU, 64) zigzag coefficients: MCUs in raster order, one DC predictor a component"""
    huff = J.huffman_codes()
    acc, nacc, raw = 0, 0, bytearray()

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
    chroma_tables = layout == "L" and "grey_chroma_table" in faults
    for mcu in zz:
        at_mcu_start = pred[0]
        for j, blk in enumerate(mcu):
            comp = COMPONENTS[layout][j]
            dc, ac = (2, 3) if comp or chroma_tables else (0, 1)
            before = at_mcu_start if (layout == "4:2:2" and j == 1 and "y1_pred_prev_mcu" in faults) else pred[comp]
            n, bits = magnitude(int(blk[0]) - before)
            pred[comp] = int(blk[0])
            put(dc, n, bits, n)
            last = 0
            for k in np.nonzero(blk[1:])[0] + 1:
                run = int(k) - last - 1
                while run > 15:
                    put(ac, 0xF0)
                    counters["zrl"] += 1
                    run -= 16
                n, bits = magnitude(int(blk[k]))
                put(ac, run << 4 | n, bits, n)
                last = int(k)
            if last < 63:
                put(ac, 0)
    pad = -nacc % 8
    counters["padded"] += pad > 0
    counters["aligned"] += pad == 0
    if pad:
        raw.append((acc << pad) | ((1 << pad) - 1))
    counters["stuffed"] += raw.count(b"\xff")
    return bytes(raw).replace(b"\xff", b"\xff\x00")


def encode_counters():
    return dict(zrl=0, stuffed=0, padded=0, aligned=0, dummies=0)


def file_restated(f, quality, layout, counters=None, faults=()):
    """the file of one frame: (H,W) uint8 for layout "L", else (H,W,3)"""
    counters = encode_counters() if counters is None else counters
    H, W = f.shape[:2]
    low = J.lower_jpeg(H, W, quality, "L" if layout == "L" else "RGB", "4:2:0" if layout == "L" else layout)
    zz, dummy = mcus_restated(f, layout, low["divisors"], faults)
    counters["dummies"] += int(dummy.sum())
    return low["header"] + stream_of(zz, layout, counters, faults) + b"\xff\xd9"


def files_restated(frames, quality, mode="RGB", subsampling="4:2:0"):
    """the files of (...,H,W,3) or (...,H,W) uint8 frames (a tensor or an array, on the host), in row-major order: what
    ``encode_jpeg(frames, quality, mode, subsampling)`` is held to.  4:2:0 is tests/test_jpeg_host.py's ``jpeg_restated``"""
    f = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    layout = J.check_layout(mode, subsampling)
    if layout == "4:2:0":
        return jpeg_restated(f, quality)
    tail = f.shape[-2:] if layout == "L" else f.shape[-3:]
    return [file_restated(one, quality, layout) for one in f.reshape((-1,) + tail)]


# ---- the restatement: decoding ------------------------------------------------------------------------------------------------------
def decode_restated(f, quality, layout, counters=None, faults=()):
    """one (H,W,3) uint8 frame as Pillow reopens its 4:4:4 or 4:2:2 file: (H,W,3) uint8"""
    counters = new_counters() if counters is None else counters
    counters["faults"] = ()                                      # (samples_restated reads its own faults there: none of ours)
    H, W = f.shape[:2]
    low = J.lower_jpeg(H, W, quality, "RGB", layout)
    my, mx = low["mcu_rows"], low["mcu_cols"]
    zz, dummy = mcus_restated(f, layout, low["divisors"])
    tables = low["qtables"].astype(np.int64)[[1 if c else 0 for c in COMPONENTS[layout]]].reshape(1, -1, 8, 8)
    s = samples_restated(natural(zz.astype(np.int64)) * tables, counters, ~dummy)
    luma = len(COMPONENTS[layout]) - 2
    y = s[:, :luma].reshape(my, mx, luma, 8, 8).transpose(0, 3, 1, 2, 4).reshape(8 * my, 8 * luma * mx)[:H, :W]
    up = []
    for j in (luma, luma + 1):
        c = s[:, j].reshape(my, mx, 8, 8).transpose(0, 2, 1, 3).reshape(8 * my, 8 * mx)[:H]
        if layout == "4:4:4":
            up.append(c[:, :W])
            continue
        wd, cols = (W + 1) // 2, np.arange(W)
        cx = cols >> 1
        if wd > 2 or "fancy_when_narrow" in faults:              # h2v1 "fancy": no vertical neighbour
            counters["fancy"] += 1
            other = np.where(cols & 1, np.minimum(cx + 1, wd - 1), np.maximum(cx - 1, 0))
            even, odd = (2, 1) if "h2v1_rounding_swapped" in faults else (1, 2)
            up.append((3 * c[:, cx] + c[:, other] + np.where(cols & 1, odd, even)) >> 2)
        else:
            counters["replicated"] += 1
            up.append(c[:, cx])
    cb, cr = up[0] - 128, up[1] - 128
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], axis=-1)
    for k in range(3):
        counters["rgb_low"][k] += int((rgb[..., k] < 0).sum())
        counters["rgb_high"][k] += int((rgb[..., k] > 255).sum())
    return np.clip(rgb, 0, 255).astype(np.uint8)


def roundtrip_restated(frames, quality, subsampling):
    """(...,H,W,3) uint8 frames -> the same shape: what ``jpeg_roundtrip(frames, quality, subsampling=subsampling)`` is held to"""
    f = frames.cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    return np.stack([decode_restated(x, quality, subsampling) for x in f.reshape((-1,) + f.shape[-3:])]).reshape(f.shape)


# ---- Pillow -------------------------------------------------------------------------------------------------------------------------
def pillow_file(f, quality, layout):
    buf = io.BytesIO()
    kw = {} if layout == "L" else dict(subsampling=layout)
    pil_image().fromarray(f).save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def pillow_reopened(f, quality, layout):
    Image = pil_image()
    with Image.open(io.BytesIO(pillow_file(f, quality, layout))) as im:
        assert im.mode == ("L" if layout == "L" else "RGB")
        return np.asarray(im.convert(im.mode))


# ---- tests: the restatement is Pillow's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_restatement_is_pillows_file(H, W, layout):
    pil_image()
    for kind in contents_of(layout):
        f = frame_of(kind, H, W, layout)
        for q in QUALITIES:
            ours, theirs = file_restated(f, q, layout), pillow_file(f, q, layout)
            assert ours == theirs, (kind, q, differ(ours, theirs))


def test_every_quality_on_one_mask():
    pil_image()
    m = grey_content("noise", 17, 23)
    for q in range(1, 101):
        assert file_restated(m, q, "L") == pillow_file(m, q, "L"), q


def test_pillows_ints_are_the_strings():
    pil_image()
    f = content("noise", 17, 23)
    for k, s in enumerate(J.SUBSAMPLINGS):
        buf = io.BytesIO()
        pil_image().fromarray(f).save(buf, "JPEG", quality=75, subsampling=k)
        assert buf.getvalue() == pillow_file(f, 75, s) and J.check_layout("RGB", k) == s
    assert files_restated(f, 75, "RGB", 2) == jpeg_restated(f, 75) == [pillow_file(f, 75, "4:2:0")]


@pytest.mark.parametrize("layout,shapes", (("4:4:4", SHAPES), ("4:2:2", DECODE_422_SHAPES)))
def test_restatement_is_pillows_reopened_file(layout, shapes):
    pil_image()
    for H, W in shapes:
        for kind in CONTENTS:
            f = content(kind, H, W)
            for q in QUALITIES:
                ours, theirs = decode_restated(f, q, layout), pillow_reopened(f, q, layout)
                assert np.array_equal(ours, theirs), (H, W, kind, q, int((ours != theirs).sum()))


# ---- tests: the cases reach what they are for -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counters_at_17x23(layout):
    enc, dec = encode_counters(), new_counters()
    for kind in contents_of(layout):
        f = frame_of(kind, 17, 23, layout)
        for q in QUALITIES:
            file_restated(f, q, layout, enc)
            if layout != "L":
                decode_restated(f, q, layout, dec)
    return enc, dec


@pytest.mark.parametrize("layout", LAYOUTS)
def test_cases_reach_every_path(layout):
    enc, dec = counters_at_17x23(layout)
    assert enc["zrl"] > 0                                        # runs of sixteen zeros
    assert enc["stuffed"] > 0                                    # a 0xFF in a stream
    assert enc["padded"] > 0 and enc["aligned"] > 0              # streams that end inside a byte and on a byte boundary
    assert (enc["dummies"] > 0) == (layout == "4:2:2")           # 23 columns: three block columns in two MCUs; never in L and 4:4:4
    if layout != "L":
        assert dec["idct_low"] > 0 and dec["idct_high"] > 0 and dec["idct_wrap"] == 0
        assert min(dec["rgb_low"]) > 0 and min(dec["rgb_high"]) > 0


def test_dummies_by_width():
    """Y1 is a dummy where 2 mx + 1 >= ceil(W / 8): W mod 16 in 1..8.  (W = 9 has two block columns in its one MCU, so none: the files of
    7 x 9 and 33 x 9 above equal Pillow's without one, and ``dummy_own_coef`` shows that a dummy more or fewer changes the file.)"""
    for W, want in ((9, False), (17, True), (23, True), (40, True), (16, False), (32, False), (8, True)):
        c = encode_counters()
        file_restated(content("noise", 9, W), 100, "4:2:2", c)
        assert (c["dummies"] > 0) == want, W                     # W mod 16 in 1..8
        for layout in ("L", "4:4:4"):
            c = encode_counters()
            file_restated(frame_of("noise", 9, W, layout), 100, layout, c)
            assert c["dummies"] == 0, (layout, W)


def test_decoder_takes_both_upsampling_branches():
    narrow, wide, none = new_counters(), new_counters(), new_counters()
    decode_restated(content("noise", 3, 4), 100, "4:2:2", narrow)
    decode_restated(content("noise", 3, 5), 100, "4:2:2", wide)
    decode_restated(content("noise", 3, 5), 100, "4:4:4", none)
    assert (narrow["fancy"], narrow["replicated"], wide["fancy"], wide["replicated"]) == (0, 2, 2, 0)     # the rule changes between W = 4 and 5
    assert (none["fancy"], none["replicated"]) == (0, 0)


# ---- tests: the yardstick can fail -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", FAULTS)
def test_the_yardstick_can_fail(fault):
    """each mistake is caught by at least one listed case, against Pillow"""
    pil_image()
    decode = fault in ("h2v1_rounding_swapped", "fancy_when_narrow")
    layout = "L" if fault == "grey_chroma_table" else "4:2:2"
    caught = 0
    for H, W in (DECODE_422_SHAPES if decode else SHAPES):
        for kind in ("noise", "ramp"):
            f = frame_of(kind, H, W, layout)
            for q in (100, 30):
                if decode:
                    theirs = pillow_reopened(f, q, layout)
                    assert np.array_equal(decode_restated(f, q, layout), theirs)
                    caught += not np.array_equal(decode_restated(f, q, layout, faults=(fault,)), theirs)
                else:
                    theirs = pillow_file(f, q, layout)
                    assert file_restated(f, q, layout) == theirs
                    caught += file_restated(f, q, layout, faults=(fault,)) != theirs
    assert caught > 0, fault


# ---- tests: headers, lower_jpeg, the ABI ----------------------------------------------------------------------------------------------
def lowered(H, W, q, layout):
    return J.lower_jpeg(H, W, q, "L" if layout == "L" else "RGB", "4:2:0" if layout == "L" else layout)


def test_headers_are_pillows():
    pil_image()
    for (H, W), q in (((1, 1), 100), ((17, 23), 75), ((128, 64), 100), ((300, 260), 30)):
        for layout in LAYOUTS + ("4:2:0",):
            head = lowered(H, W, q, layout)["header"]
            theirs = pillow_file(np.zeros((H, W) if layout == "L" else (H, W, 3), dtype=np.uint8), q, layout)
            assert theirs[:len(head)] == head and len(head) == (328 if layout == "L" else 623), (H, W, q, layout)


def test_header_segments():
    grey, c444, c422, c420 = (lowered(17, 23, 75, layout)["header"] for layout in ("L", "4:4:4", "4:2:2", "4:2:0"))
    assert grey.count(b"\xff\xdb\x00\x43") == 1 and grey.count(b"\xff\xc4") == 2
    sof = grey.index(b"\xff\xc0")
    assert grey[sof + 2:sof + 13] == b"\x00\x0b\x08\x00\x11\x00\x17\x01\x01\x11\x00"
    assert grey.endswith(b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00")
    sof = c420.index(b"\xff\xc0")
    assert (c444[sof + 11], c422[sof + 11], c420[sof + 11]) == (0x11, 0x21, 0x22)
    for other in (c444, c422):                                   # nothing else differs
        assert len(other) == len(c420) and [i for i in range(len(c420)) if other[i] != c420[i]] == [sof + 11]


def test_lower_jpeg_defaults_are_unchanged():
    for (H, W), q in (((17, 23), 75), ((256, 256), 100), ((1, 1), 1)):
        low = J.lower_jpeg(H, W, q)
        assert low is J.lower_jpeg(H, W, q, "RGB", "4:2:0") and low is J.lower_jpeg(H, W, q, mode="RGB", subsampling=2)
        my, mx = (H + 15) // 16, (W + 15) // 16
        chunks = (6 * my * mx * 208 + 1023) // 1024
        assert (low["H"], low["W"], low["quality"], low["mcu_rows"], low["mcu_cols"], low["blocks"], low["chunks"]) == (H, W, q, my, mx, 6 * my * mx, chunks)
        assert (low["blocks_per_mcu"], low["mcu_height"], low["mcu_width"], low["mode"], low["subsampling"]) == (6, 16, 16, "RGB", "4:2:0")
        assert low["header"] == J.header_bytes(H, W, J.quant_tables(q)) and len(low["header"]) == 623
        assert low["stream_capacity"] == chunks * 1024 and low["file_capacity"] == 623 + 2 * chunks * 1024 + 2
        assert np.array_equal(low["qtables"], J.quant_tables(q)) and np.array_equal(low["divisors"], 8 * J.quant_tables(q))
        want = np.concatenate([(8 * J.quant_tables(q)).reshape(-1), J.huffman_codes().reshape(-1),
                               np.frombuffer(low["header"] + b"\0", dtype=np.uint8).view(np.int32)])
        assert low["params"].dtype == torch.int32 and np.array_equal(low["params"].numpy(), want)
    assert J.lower_jpeg(256, 256, 100)["blocks"] == 1536


@pytest.mark.parametrize("layout", LAYOUTS + ("4:2:0",))
def test_lower_jpeg_layouts_and_the_librarys_queries(layout):
    import ctypes
    N = importlib.import_module("3d-magic-mirror_amd._native")
    L = N.lib()
    per, mh, mw = {"L": (1, 8, 8), "4:4:4": (3, 8, 8), "4:2:2": (4, 8, 16), "4:2:0": (6, 16, 16)}[layout]
    for H, W in ((17, 23), (128, 64), (1, 1), (136, 128)):
        low = lowered(H, W, 75, layout)
        my, mx = -(-H // mh), -(-W // mw)
        assert (low["blocks_per_mcu"], low["mcu_height"], low["mcu_width"], low["mcu_rows"], low["mcu_cols"], low["blocks"]) == (per, mh, mw, my, mx, per * my * mx)
        assert low["chunks"] == (low["blocks"] * 208 + 1023) // 1024 and low["stream_capacity"] == 1024 * low["chunks"]
        assert low["file_capacity"] == len(low["header"]) + 2 * low["stream_capacity"] + 2
        assert low["params"].numel() == 128 + 1024 + (len(low["header"]) + 3) // 4
        assert bytes(low["params"][128 + 1024:].numpy().view(np.uint8)[:len(low["header"])]) == low["header"]
        assert np.array_equal(low["params"][:128 + 1024].numpy(), J.lower_jpeg(H, W, 75)["params"][:128 + 1024].numpy())
        d = N.MMJpegModesDesc()
        d.H, d.W, d.header_bytes, d.mode, d.sampling = H, W, len(low["header"]), J.MODES[low["mode"]], J.SAMPLINGS[layout]
        for n in (1, 3, 48):
            d.n = n
            assert L.mm_jpeg_modes_query_workspace(ctypes.byref(d)) == low["workspace_bytes"](n) > n * low["file_capacity"]
            assert L.mm_jpeg_modes_files_offset(ctypes.byref(d)) == low["files_offset"](n)
            assert L.mm_jpeg_modes_coef_offset(ctypes.byref(d)) == low["coef_offset"](n) > low["files_offset"](n)
            assert low["coef_offset"](n) + n * low["blocks"] * 128 <= low["workspace_bytes"](n)
            if layout == "L":
                continue
            r = N.MMJpegRoundtripDesc()
            r.n, r.H, r.W, r.mode, r.sampling = n, H, W, N.JPEG_MODE_RGB, J.SAMPLINGS[layout]
            assert L.mm_jpeg_roundtrip_query_workspace(ctypes.byref(r)) == low["roundtrip_workspace_bytes"](n) >= n * my * mx * (per * 128 + mh * mw + 128)
            r.coef = ctypes.c_void_p(16)
            assert L.mm_jpeg_roundtrip_query_workspace(ctypes.byref(r)) == low["roundtrip_workspace_bytes"](n, own_coef=False)
    with pytest.raises(ValueError):
        lowered(65536, 8, 75, layout)


def test_block_limits_count_the_layouts_own_blocks():
    """8192 x 8192 has 2^20 blocks as a mask (allowed) and three times as many in 4:4:4 (refused): Python and the library agree"""
    import ctypes
    N = importlib.import_module("3d-magic-mirror_amd._native")
    L = N.lib()
    assert J.lower_jpeg(8192, 8192, 100, "L")["blocks"] == J.MAX_BLOCKS
    for sub in J.SUBSAMPLINGS:                                   # 3, 2 and 1.5 blocks per 8 x 8 pixels
        with pytest.raises(ValueError, match="blocks"):
            J.lower_jpeg(8192, 8192, 100, "RGB", sub)
    assert J.lower_jpeg(8192, 4096, 100, "RGB", "4:2:2")["blocks"] == J.MAX_BLOCKS
    d = N.MMJpegModesDesc()
    d.n, d.H, d.W, d.header_bytes = 1, 8192, 8192, 328
    d.frames = d.params = d.params_host = d.workspace = ctypes.c_void_p(16)
    d.mode = N.JPEG_MODE_L
    assert L.mm_jpeg_modes_query_workspace(ctypes.byref(d)) == J.lower_jpeg(8192, 8192, 100, "L")["workspace_bytes"](1)
    d.mode, d.header_bytes = N.JPEG_MODE_RGB, 623
    for sampling in (N.JPEG_SAMPLING_444, N.JPEG_SAMPLING_422, N.JPEG_SAMPLING_420):
        d.sampling = sampling
        assert L.mm_jpeg_modes_query_workspace(ctypes.byref(d)) == 0 and L.mm_jpeg_modes_encode(ctypes.byref(d), None) == -5
    d.W, d.sampling = 4096, N.JPEG_SAMPLING_422
    assert L.mm_jpeg_modes_query_workspace(ctypes.byref(d)) == J.lower_jpeg(8192, 4096, 100, "RGB", "4:2:2")["workspace_bytes"](1)


def test_argument_errors(pkg):
    ok, mask = torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 8, 8), dtype=torch.uint8)
    for fn in (pkg.encode_jpeg, pkg.jpeg_roundtrip):
        with pytest.raises(ValueError, match="H,W,3"):           # the wrong channel count for the mode
            fn(mask)
        with pytest.raises(ValueError, match="H,W,3"):
            fn(mask, subsampling="4:4:4")
        with pytest.raises(ValueError, match=r"\(\.\.\.,H,W\)"):
            fn(torch.zeros((8,), dtype=torch.uint8), mode="L")
        for sub in ("4:4:4", "4:2:2", 0, 1):
            with pytest.raises(ValueError, match="subsampling"):
                fn(mask, mode="L", subsampling=sub)
        for sub in ("4:1:1", "4:4:0", "444", "", None, 3, -1, 1.0, True):
            with pytest.raises(ValueError, match="subsampling"):
                fn(ok, subsampling=sub)
        for mode in ("rgb", "YCbCr", "l", None, 0):
            with pytest.raises(ValueError, match="mode"):
                fn(ok, mode=mode)
        for x, kw in ((mask, dict(mode="L")), (ok, dict(subsampling="4:2:2")), (ok, dict(subsampling=0)), (mask, dict(mode="L", subsampling=2))):
            with pytest.raises(ValueError, match="uint8"):
                fn(x.int(), **kw)
            with pytest.raises(ValueError, match="quality"):
                fn(x, quality=0, **kw)
            with pytest.raises(RuntimeError, match="device"):    # every argument is fine: a host tensor, and there is no CPU fallback
                fn(x, **kw)
    with pytest.raises(ValueError, match="export_images"):
        pkg.encode_jpeg(mask.float(), mode="L")
    with pytest.raises(ValueError, match="empty"):
        pkg.encode_jpeg(mask[:0], mode="L")
    with pytest.raises(ValueError, match="files=True"):
        pkg.jpeg_roundtrip(mask, mode="L", files=True)
    for kw in (dict(mode="L", subsampling="4:4:4"), dict(subsampling="4:1:1"), dict(mode="CMYK")):
        with pytest.raises(ValueError):
            J.lower_jpeg(8, 8, 100, **kw)
    with pytest.raises(ValueError, match="B,4,H,W"):
        pkg.recon_scores_as_saved(torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8), files=True)


def test_abi_mirror_and_return_codes():
    import ctypes
    N = importlib.import_module("3d-magic-mirror_amd._native")
    L = N.lib()
    assert L.mm_abi_version() == 9 == N.ABI_VERSION              # additions only: the version stays
    assert L.mm_struct_size(42) == ctypes.sizeof(N.MMJpegModesDesc) > 0 and N.STRUCT_IDS[42] is N.MMJpegModesDesc
    assert L.mm_struct_size(37) == ctypes.sizeof(N.MMJpegDesc) and L.mm_struct_size(38) == ctypes.sizeof(N.MMJpegRoundtripDesc)
    assert {"mm_jpeg_modes_query_workspace", "mm_jpeg_modes_files_offset", "mm_jpeg_modes_coef_offset", "mm_jpeg_modes_encode"} <= set(N.EXPORTS)
    assert (N.JPEG_SAMPLING_420, N.JPEG_SAMPLING_422, N.JPEG_SAMPLING_444) == (0, 1, 2)
    keep = ctypes.create_string_buffer(64)
    fake = ctypes.c_void_p(ctypes.addressof(keep) + 15 & ~15)    # never dereferenced: every refusal comes before any GPU work
    lows = {layout: lowered(17, 23, 75, layout) for layout in LAYOUTS + ("4:2:0",)}
    pars = {layout: low["params"].numpy().copy() for layout, low in lows.items()}

    def desc(layout="L", n=3, H=17, W=23, mode=None, sampling=None, params=None):
        d = N.MMJpegModesDesc()
        d.n, d.H, d.W, d.header_bytes = n, H, W, len(lows[layout]["header"])
        d.mode = J.MODES[lows[layout]["mode"]] if mode is None else mode
        d.sampling = J.SAMPLINGS[layout] if sampling is None else sampling
        d.frames = d.params = d.workspace = fake
        d.params_host = ctypes.c_void_p((pars[layout] if params is None else params).ctypes.data)
        d.workspace_bytes = L.mm_jpeg_modes_query_workspace(ctypes.byref(d))
        return d

    assert L.mm_jpeg_modes_encode(None, None) == -1 and L.mm_jpeg_modes_query_workspace(None) == 0
    for layout in lows:
        d = desc(layout)
        assert d.workspace_bytes == lows[layout]["workspace_bytes"](3)
        d.frames = None
        assert L.mm_jpeg_modes_encode(ctypes.byref(d), None) == -1, layout
        for kw in (dict(n=0), dict(H=0), dict(W=-1)):
            d = desc(layout, **kw)
            assert L.mm_jpeg_modes_encode(ctypes.byref(d), None) == -2 and d.workspace_bytes == 0, (layout, kw)
        for kw in (dict(H=65536), dict(n=65536)):
            d = desc(layout, **kw)
            assert L.mm_jpeg_modes_encode(ctypes.byref(d), None) == -5 and d.workspace_bytes == 0, (layout, kw)
        d = desc(layout)
        d.workspace_bytes -= 1
        assert L.mm_jpeg_modes_encode(ctypes.byref(d), None) == -3, layout
        bad = pars[layout].copy()
        bad[5] = 12                                              # a divisor that is not 8 * (1..255)
        assert L.mm_jpeg_modes_encode(ctypes.byref(desc(layout, params=bad)), None) == -2, layout
    # an unknown mode or sampling, a sampling with mode L: -2 from the encoder, 0 from its queries, and the same from the round trip
    refused = (dict(mode=2), dict(mode=-1), dict(mode=N.JPEG_MODE_RGB, sampling=3), dict(mode=N.JPEG_MODE_RGB, sampling=-1),
               dict(mode=N.JPEG_MODE_L, sampling=N.JPEG_SAMPLING_444), dict(mode=N.JPEG_MODE_L, sampling=N.JPEG_SAMPLING_422))
    for kw in refused:
        d = desc("4:2:0", **kw)
        assert L.mm_jpeg_modes_encode(ctypes.byref(d), None) == -2 and d.workspace_bytes == 0, kw
        assert L.mm_jpeg_modes_files_offset(ctypes.byref(d)) == 0 and L.mm_jpeg_modes_coef_offset(ctypes.byref(d)) == 0, kw
        r = N.MMJpegRoundtripDesc()
        r.n, r.H, r.W, r.mode, r.sampling = 3, 17, 23, kw["mode"], kw.get("sampling", 0)
        r.frames = r.params = r.out = r.workspace = fake
        r.params_host = ctypes.c_void_p(pars["4:2:0"].ctypes.data)
        assert L.mm_jpeg_roundtrip_query_workspace(ctypes.byref(r)) == 0 and L.mm_jpeg_roundtrip(ctypes.byref(r), None) == -2, kw
    # MMJpegDesc is the new descriptor with mode RGB and sampling 4:2:0
    e = N.MMJpegDesc()
    e.n, e.H, e.W, e.header_bytes = 3, 17, 23, 623
    d = desc("4:2:0")
    for old, new in (("mm_jpeg_query_workspace", "mm_jpeg_modes_query_workspace"), ("mm_jpeg_files_offset", "mm_jpeg_modes_files_offset"),
                     ("mm_jpeg_coef_offset", "mm_jpeg_modes_coef_offset")):
        assert getattr(L, old)(ctypes.byref(e)) == getattr(L, new)(ctypes.byref(d)) > 0
