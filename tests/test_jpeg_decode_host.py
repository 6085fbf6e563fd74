"""Host side of the JPEG file decoder (3d-magic-mirror_amd/jpeg_decode.py, csrc/mm_jpeg_decode.hip), no GPU.

``decode_jpeg_host`` -- the parser, the entropy decoder and the back half restated in numpy / Python in the kernels' order -- is held to
Pillow on whole arrays with no tolerance: to the pixels recorded in tests/golden/jpeg_decode.npz (files Pillow wrote, pixels Pillow read
back) and, where Pillow imports, to live Pillow on those files and on 50 seeded random files over the accepted options.  The lowering's
records, segment tables and deduplicated tables are checked on the fixture; every rejection raises ValueError with the file's index; the
library's descriptor validation is called through ctypes.

Damaged streams run on the CPU only: tools/jpeg_entropy_check.cpp compiles csrc/mm_jpeg_entropy.h -- the very text of the kernel's segment
decoder -- into a stand-alone program under AddressSanitizer and UBSan, and every fixture file goes through it truncated at every byte of
its scan, with each single scan byte set to FF, and with 200 seeded single-byte flips.  The program must exit clean, and its per-segment
statuses and coefficients must be ``entropy_decode_host``'s (which decodes a damaged variant from the last MCU before the damage: the
bytes its reader had fetched by then are the undamaged segment's, so its state there is too; the program decodes every variant whole)."""
import bisect
import ctypes
import functools
import importlib
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

JD = importlib.import_module("3d-magic-mirror_amd.jpeg_decode")
N = importlib.import_module("3d-magic-mirror_amd._native")

try:
    from PIL import Image
except ImportError:
    Image = None


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "jpeg_decode.npz"))
    return {k: z[k] for k in z.files}


def names():
    return [str(n) for n in fixture()["names"]]


def file_of(name):
    return bytes(fixture()["file_" + name])


def pillow(data, mode="RGB"):
    return np.asarray(Image.open(io.BytesIO(data)).convert(mode))


NAMES = names()
GREY = [n for n in NAMES if "l_" + n in fixture()]


# ---- the restatement is Pillow ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_decoder_equals_the_fixture(name):
    frames, status = JD.decode_jpeg_host([file_of(name)])
    assert status.tolist() == [0]
    assert np.array_equal(frames[0], fixture()["rgb_" + name])
    if Image is not None:
        assert np.array_equal(frames[0], pillow(file_of(name)))
    if name in GREY:
        frames, status = JD.decode_jpeg_host([file_of(name)], "L")
        assert status.tolist() == [0] and np.array_equal(frames[0], fixture()["l_" + name])


def test_host_decoder_mixed_batch_both_orders():
    for order in (NAMES, NAMES[::-1]):
        frames, status = JD.decode_jpeg_host([file_of(n) for n in order])
        assert not status.any()
        for f, n in zip(frames, order):
            assert np.array_equal(f, fixture()["rgb_" + n]), n


def test_fixture_has_what_it_is_for():
    scans = {n: file_of(n)[file_of(n).index(b"\xff\xda"):] for n in NAMES}
    assert any(b"\xff\x00" in s for s in scans.values())                        # stuffing
    assert b"\xff\xd7" in scans["rst1_420_48x80_noise"] and scans["rst1_420_48x80_noise"].count(b"\xff\xd0") >= 2      # the marker number wraps
    assert b"\xff\xfe" in file_of("comment_dpi_12x10")


def random_file(rng):
    """one file over the accepted options, as Pillow writes it: (bytes, mode)"""
    h, w = (int(v) for v in rng.integers(1, 50, 2))
    grey = rng.random() < 0.25
    img = rng.integers(0, 256, (h, w) if grey else (h, w, 3), dtype=np.uint8)
    if rng.random() < 0.5:                                                     # smoother content: long zero runs, EOBs, small categories
        img = np.sort(img, axis=1)
    kw = dict(quality=int(rng.choice([1, 10, 30, 50, 75, 90, 95, 100])), optimize=bool(rng.random() < 0.5))
    if not grey:
        kw["subsampling"] = int(rng.integers(0, 3))
    r = rng.random()
    if r < 0.25:
        kw["restart_marker_blocks"] = int(rng.integers(1, 6))
    elif r < 0.4:
        kw["restart_marker_rows"] = 1
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", **kw)
    return f.getvalue()


def test_host_decoder_equals_live_pillow_on_random_files():
    if Image is None:
        pytest.skip("Pillow is not installed: the fixture is the yardstick")
    rng = np.random.default_rng(50)
    files = [random_file(rng) for _ in range(50)]
    frames, status = JD.decode_jpeg_host(files)
    assert not status.any()
    for i, (f, data) in enumerate(zip(frames, files)):
        assert np.array_equal(f, pillow(data)), "file %d" % i
    low = JD.lower_jpeg_decode(files)
    assert len(low["sets"]) > 3 and len(low["htables"]) > 8                     # optimised tables: many sets in one batch


# ---- the lowering ------------------------------------------------------------------------------------------------------------------------
def test_lowering_of_the_fixture():
    files = [file_of(n) for n in NAMES]
    low = JD.lower_jpeg_decode(files)
    n = len(files)
    assert low["n"] == n and low["data"].tobytes() == b"".join(files)
    shapes = np.array([fixture()["rgb_" + m].shape[:2] for m in NAMES])
    assert np.array_equal(low["sizes"], shapes) and np.array_equal(low["files"][:, :2], shapes)
    assert np.array_equal(low["offsets"], np.concatenate([[0], np.cumsum(shapes[:, 0] * shapes[:, 1])]))
    layout = {m: l for m, l in zip(NAMES, low["files"][:, JD.F_LAYOUT].tolist())}
    assert layout["std_420_q75_17x23"] == 0 and layout["std_422_q85_16x33"] == 1 and layout["opt_444_q60_9x9_noise"] == 2 and layout["grey_q75_13x21"] == 3
    block0 = plane = 0
    for rec in low["files"].tolist():
        per, _, mw, mh = JD.SHAPES[rec[JD.F_LAYOUT]]
        assert rec[JD.F_MX] == -(-rec[JD.F_W] // mw) and rec[JD.F_MY] == -(-rec[JD.F_H] // mh)
        assert rec[JD.F_BLOCK0] == block0 and rec[JD.F_YOFF] == plane
        mcus = rec[JD.F_MX] * rec[JD.F_MY]
        block0, plane = block0 + mcus * per, plane + mcus * mw * mh
        if rec[JD.F_LAYOUT] != 3:
            assert rec[JD.F_COFF] == plane
            plane += mcus * 128
        assert rec[JD.F_Q0 + 3:] == [0] * (JD.FILE_INTS - JD.F_Q0 - 3)
    assert low["blocks"] == block0 and low["plane_bytes"] == plane
    assert low["workspace_bytes"] == N.up256(block0 * 128) + N.up256(4 * n) + N.up256(plane)
    # segments: grouped by set, groups padded to GROUP with count-0 rows; the live rows of a file tile its MCUs in order, their bytes ascend inside the file
    seg = low["segments"]
    assert seg.shape[0] % JD.GROUP == 0 and (seg.reshape(-1, JD.GROUP, 6)[:, :, JD.S_SET] == seg.reshape(-1, JD.GROUP, 6)[:, :1, JD.S_SET]).all()
    assert (np.diff(seg[:, JD.S_SET]) >= 0).all()
    live = seg[seg[:, JD.S_COUNT] > 0]
    want = {"rst1_420_48x80_noise": 15, "rstrow_444_24x24": 3, "grey_opt_rst3_33x17": 5}
    for i, m in enumerate(NAMES):
        rows = live[live[:, JD.S_FILE] == i]
        assert len(rows) == want.get(m, 1), m
        assert rows[0, JD.S_FIRST] == 0 and np.array_equal(rows[1:, JD.S_FIRST], np.cumsum(rows[:-1, JD.S_COUNT]))
        assert rows[:, JD.S_COUNT].sum() == low["files"][i, JD.F_MX] * low["files"][i, JD.F_MY]
        assert rows[0, JD.S_BEGIN] == low["starts"][i] + files[i].index(b"\xff\xda") + 2 + (8 if low["files"][i, JD.F_LAYOUT] == 3 else 12)
        assert (rows[:, JD.S_BEGIN] <= rows[:, JD.S_END]).all() and np.array_equal(rows[1:, JD.S_BEGIN], rows[:-1, JD.S_END] + 2)
        assert rows[-1, JD.S_END] == low["starts"][i + 1] - 2                      # EOI
    # deduplication: the six standard-table colour files share one set and four tables; the quality-75 luma table occurs once
    std = [i for i, m in enumerate(NAMES) if m.startswith(("std_", "rst1_", "rstrow_", "weblow", "q1_", "q100_", "one_", "market", "comment"))]
    assert len({int(live[live[:, JD.S_FILE] == i][0, JD.S_SET]) for i in std}) == 1
    assert len({tuple(q) for q in low["qtables"].tolist()}) == len(low["qtables"])
    assert len({t.tobytes() for t in low["htables"]}) == len(low["htables"])
    assert low["htables"].shape[1] == JD.TABLE_WORDS and low["sets"].shape[1] == JD.SET_INTS
    q75 = importlib.import_module("3d-magic-mirror_amd.jpeg").quant_tables(75)
    assert sum(np.array_equal(q, q75[0]) for q in low["qtables"]) == 1
    assert low["tables"].dtype == np.int32 and low["tables"].size == n * 16 + 2 * (n + 1) + seg.size + low["qtables"].size + low["htables"].size + low["sets"].size


def test_huffman_decode_table_of_the_standard_dc_table():
    J = importlib.import_module("3d-magic-mirror_amd.jpeg")
    _, bits, vals = J.HUFFMAN[0]
    t = JD.huffman_decode_table(bytes(bits), vals)
    look = t[:256].view(np.uint16)
    assert look[0] == (2 << 8 | 0) and look[0b010 << 6] == (3 << 8 | 1) and look[0b111111110] == (9 << 8 | 11) and look[0b111111111] == 0
    assert t[256:274].view(np.int32).tolist()[1:10] == [-1, 0, 6, 14, 30, 62, 126, 254, 510]
    assert JD.huffman_decode_table(bytes([3] + [0] * 15), b"\0\1\2") is None      # three codes of one bit


# ---- rejections ---------------------------------------------------------------------------------------------------------------------------
def patched(data, marker, at, value, count=0):
    """the file with byte ``at`` of the body of its count-th segment ``marker`` set to ``value``"""
    pos = -1
    for _ in range(count + 1):
        pos = data.index(bytes((0xFF, marker)), pos + 1)
    out = bytearray(data)
    out[pos + 4 + at] = value
    return bytes(out)


def rejected():
    base, grey = file_of("std_420_q75_17x23"), file_of("grey_q75_13x21")
    sof = base.index(b"\xff\xc0")
    sos = base.index(b"\xff\xda")
    cases = {
        "extended": base[:sof + 1] + b"\xc1" + base[sof + 2:],
        "progressive": base[:sof + 1] + b"\xc2" + base[sof + 2:],
        "12-bit": patched(base, 0xC0, 0, 12),
        "16-bit DQT": patched(base, 0xDB, 0, 0x10),
        "more than one scan": base[:-2] + base[sos:],
        "non-interleaved": base[:sos] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + base[sos + 14:],
        "DNL": patched(patched(base, 0xC0, 1, 0), 0xC0, 2, 0),
        "a DNL marker": base[:-2] + b"\xff\xdc\x00\x04\x00\x11\xff\xd9",
        "4:4:0": patched(base, 0xC0, 7, 0x12),
        "4:1:1": patched(base, 0xC0, 7, 0x41),
        "chroma 2x1": patched(base, 0xC0, 10, 0x21),
        "2 components": base[:sof + 2] + b"\x00\x0e" + base[sof + 4:sof + 9] + b"\x02" + base[sof + 10:sof + 16] + base[sof + 19:],
        "4 components": base[:sof + 2] + b"\x00\x14" + base[sof + 4:sof + 9] + b"\x04" + base[sof + 10:sof + 19] + b"\x04\x11\x01" + base[sof + 19:],
        "Adobe transform 0": base[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + base[2:],
        "ids R, G, B": patched(patched(patched(base, 0xC0, 6, 0x52), 0xC0, 9, 0x47), 0xC0, 12, 0x42),
        "undefined Huffman table": patched(grey, 0xDA, 2, 0x01),               # AC table 1 in a greyscale file, which defines DC 0 and AC 0 only
        "undefined quantisation table": patched(base, 0xC0, 8, 3),
        "length past the file": patched(base, 0xE0, -2, 0xFF),
        "no SOI": base[2:],
        "no SOF": base[:sof] + base[sos:],
        "no SOS": base[:sos],
        "Huffman id 2": patched(base, 0xC4, 0, 0x02),
        "oversubscribed DHT": patched(base, 0xC4, 1, 3),
        "not bytes": 17,
    }
    return cases


WORDS = {"extended": "extended", "progressive": "progressive"}


@pytest.mark.parametrize("why", sorted(rejected()))
def test_parser_rejects(why):
    good = file_of("q100_8x8_noise")
    with pytest.raises(ValueError, match=r"file 2\b") as e:
        JD.lower_jpeg_decode([good, good, rejected()[why], good])
    if why in WORDS:
        assert WORDS[why] in str(e.value)


def test_parser_rejects_pillows_progressive_file():
    """(Pillow cannot write 4:1:1: its subsampling="4:1:1" is a legacy spelling of 4:2:0, luma 2x2 -- asserted here -- so the 4:1:1 and 4:4:0
    files of ``rejected`` are patched headers)"""
    if Image is None:
        pytest.skip("Pillow is not installed")
    img = np.random.default_rng(3).integers(0, 256, (24, 40, 3), dtype=np.uint8)
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", progressive=True)
    with pytest.raises(ValueError, match=r"file 1: .*progressive"):
        JD.lower_jpeg_decode([file_of("one_pixel"), f.getvalue()])
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", subsampling="4:1:1")
    assert JD.parse_header(f.getvalue())["layout"] == 0


def test_mode_l_is_for_greyscale_files_only():
    with pytest.raises(ValueError, match=r"file 1: a colour file with mode 'L'"):
        JD.lower_jpeg_decode([file_of("grey_q75_13x21"), file_of("one_pixel")], "L")
    with pytest.raises(ValueError, match="mode"):
        JD.lower_jpeg_decode([file_of("one_pixel")], "YCbCr")
    with pytest.raises(ValueError, match="empty"):
        JD.lower_jpeg_decode([])


def test_tolerated_oddities_decode_like_the_plain_file():
    base = file_of("std_420_q75_17x23")
    want = fixture()["rgb_std_420_q75_17x23"]
    sos = base.index(b"\xff\xda")
    forms = {"bytes after EOI": base + b"trailing \xff\xd8 bytes", "no EOI": base[:-2], "fill bytes before markers": base[:sos] + b"\xff\xff\xff" + base[sos:-2] + b"\xff\xff\xff\xd9",
             "bytearray": bytearray(base)}
    for what, data in forms.items():
        frames, status = JD.decode_jpeg_host([data])
        assert status.tolist() == [0] and np.array_equal(frames[0], want), what


def test_paths_and_jpeg_batches_are_files(tmp_path):
    J = importlib.import_module("3d-magic-mirror_amd.jpeg")
    p = tmp_path / "a.jpg"
    p.write_bytes(file_of("one_pixel"))
    a = JD.lower_jpeg_decode([str(p), p])
    assert a["data"].tobytes() == 2 * file_of("one_pixel")
    both = file_of("one_pixel") + file_of("q100_8x8_noise")
    b = JD.lower_jpeg_decode(J.JpegBatch(np.frombuffer(both + b"slack", dtype=np.uint8), [0, len(file_of("one_pixel")), len(both)]))
    assert b["n"] == 2 and np.array_equal(b["sizes"], [[1, 1], [8, 8]]) and b["data"].size == len(both)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def descriptor(low, keep):
    d = N.MMJpegDecodeDesc()
    d.n, d.mode, d.n_segments = low["n"], JD.MODES[low["mode"]], low["segments"].shape[0]
    d.n_qtables, d.n_htables, d.n_sets, d.n_bytes = low["qtables"].shape[0], low["htables"].shape[0], low["sets"].shape[0], low["data"].size
    tables = np.ascontiguousarray(low["tables"])
    keep.append(tables)
    d.tables_host = tables.ctypes.data
    return d, tables


def test_struct_size_and_query_workspace():
    lib = N.lib()
    assert lib.mm_struct_size(45) == ctypes.sizeof(N.MMJpegDecodeDesc) != 0 and N.STRUCT_IDS[45] is N.MMJpegDecodeDesc
    keep = []
    for files, mode in (([file_of(n) for n in NAMES], "RGB"), ([file_of(n) for n in GREY], "L"), ([file_of("one_pixel")], "RGB")):
        low = JD.lower_jpeg_decode(files, mode)
        d, _ = descriptor(low, keep)
        assert N.fn("mm_jpeg_decode_query_workspace")(d) == low["workspace_bytes"]


def test_descriptor_validation_return_codes():
    """every refusal comes before any launch: the pointers below are never dereferenced on a device (the call returns at the check)"""
    keep = []
    low = JD.lower_jpeg_decode([file_of(n) for n in NAMES])
    call, query = N.fn("mm_jpeg_decode"), N.fn("mm_jpeg_decode_query_workspace")
    T = JD
    t_files, t_off = 0, low["n"] * 16
    t_seg = t_off + 2 * (low["n"] + 1)
    t_q = t_seg + low["segments"].size
    t_h = t_q + low["qtables"].size
    t_sets = t_h + low["htables"].size
    live = int(np.flatnonzero(low["segments"][:, T.S_COUNT] > 0)[3])
    BAD, UNSUP, NULL = -2, -5, -1

    def status(edit=None, **fields):
        d, tables = descriptor(low, keep)
        if edit:
            edit(tables)
        for k, v in fields.items():
            setattr(d, k, v)
        st = call(d, None)
        assert (query(d) == 0) == (st != NULL or not d.tables_host), (st, query(d))          # the query answers 0 for whatever the call refuses
        return st

    def put(at, value):
        return lambda t: t.__setitem__(at, value)

    assert status() == NULL                                                      # the tables pass; bytes, tables, out and workspace are NULL
    assert status(n=0) == BAD and status(n_segments=low["segments"].shape[0] - 1) == BAD and status(n_segments=0) == BAD
    assert status(mode=2) == BAD and status(n_bytes=0) == BAD and status(n_qtables=0) == BAD
    assert status(n_bytes=1 << 31) == UNSUP and status(tables_host=None) == NULL
    assert status(put(t_files + T.F_H, 0)) == BAD and status(put(t_files + T.F_W, 70000)) == BAD and status(put(t_files + T.F_LAYOUT, 4)) == BAD
    assert status(put(t_files + T.F_MX, 1)) == BAD and status(put(t_files + 16 + T.F_BLOCK0, 1)) == BAD and status(put(t_files + 16 + T.F_YOFF, 64)) == BAD
    assert status(put(t_files + T.F_COFF, 0)) == BAD and status(put(t_files + T.F_Q0 + 1, low["qtables"].shape[0])) == BAD and status(put(t_files + T.F_Q0, -1)) == BAD
    assert status(put(t_off + 2, 1)) == BAD and status(put(t_off, 1)) == BAD                          # offsets that are not the running sum
    s0 = t_seg + 6 * live
    assert status(put(s0 + T.S_FILE, low["n"])) == BAD and status(put(s0 + T.S_FIRST, -1)) == BAD and status(put(s0 + T.S_COUNT, 1 << 20)) == BAD
    assert status(put(s0 + T.S_BEGIN, -1)) == BAD and status(put(s0 + T.S_END, low["data"].size + 1)) == BAD
    assert status(lambda t: (t.__setitem__(s0 + T.S_BEGIN, 9), t.__setitem__(s0 + T.S_END, 8))) == BAD    # not begin <= end
    assert status(put(s0 + T.S_SET, len(low["sets"]))) == BAD
    if len(low["sets"]) > 1:
        assert status(put(s0 + T.S_SET, 1 - int(low["segments"][live, T.S_SET]))) == BAD               # mixed sets in a workgroup
    assert status(put(t_q + 5, 0)) == BAD and status(put(t_q + 5, 256)) == BAD
    assert status(put(t_sets + 2, low["htables"].shape[0])) == BAD and status(put(t_sets, -1)) == BAD
    lowl = JD.lower_jpeg_decode([file_of("grey_q75_13x21"), file_of("one_pixel")])
    d, _ = descriptor(lowl, keep)
    d.mode = N.JPEG_MODE_L
    assert call(d, None) == BAD                                                  # a colour record in mode L


# ---- damaged streams: the kernel's segment decoder under the host sanitizers ----------------------------------------------------------------
def checker(tmp):
    """tools/jpeg_entropy_check.cpp built with the host sanitizers: (path, "") or (None, why the sanitizers cannot be linked here).  The
    program itself must compile: a plain build that fails is an error, not a skip."""
    exe = os.path.join(tmp, "jpeg_entropy_check")
    base = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "3d-magic-mirror_amd", "csrc"),
            os.path.join(ROOT, "tools", "jpeg_entropy_check.cpp"), "-o", exe]
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr[-2000:]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    return (exe, "") if r.returncode == 0 else (None, r.stderr[-400:])


def checksum(coef):
    """the program's: the sum over i of (coefficient i as uint16 + 1) * (i * 0x9E3779B97F4A7C15 + 1), modulo 2^64"""
    with np.errstate(over="ignore"):
        i = np.arange(coef.size, dtype=np.uint64)
        return "%016x" % int(((coef.reshape(-1).view(np.uint16).astype(np.uint64) + np.uint64(1)) * (i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1))).sum(dtype=np.uint64))


def bad_code_edits(scan):
    """the scan's first bytes as FF 00 FF 00, sixteen 1-bits: no DC code of the standard (or of any complete) table is all ones"""
    return ((scan, 0xFF), (scan + 1, 0), (scan + 2, 0xFF), (scan + 3, 0))


def damaged_forms(data, scan, rng):
    """(length, edits) of every damaged form of one file: truncated at every byte of its scan, each scan byte set to FF, 200 single flips,
    and one made to end in BAD_CODE (the standard tables leave only all-ones codes unassigned, which a single flip rarely makes)"""
    forms = [(k, ()) for k in range(scan, len(data))]
    forms += [(len(data), ((k, 0xFF),)) for k in range(scan, len(data))]
    forms += [(len(data), ((int(rng.integers(scan, len(data))), int(rng.integers(0, 256))),)) for _ in range(200)]
    return forms + [(len(data), bad_code_edits(scan))]


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe, why = checker(str(tmp_path_factory.mktemp("entropy")))
    if exe is None:
        pytest.skip("g++ -fsanitize=address,undefined cannot build here: " + why)
    return exe


def run_forms(exe, tmp, name, forms, data=None):
    """one fixture file's forms (or those of ``data``, a clean file, under ``name``) through the sanitized program and through
    ``entropy_decode_host``: [(form, statuses, status of the file)]"""
    data = file_of(name) if data is None else data
    h = JD.parse_header(data)
    per, luma = JD.SHAPES[h["layout"]][:2]
    mcus, blocks = h["mx"] * h["my"], h["mx"] * h["my"] * per
    low = JD.lower_jpeg_decode([data])
    sets, lists = low["sets"][0], [JD._table_lists(t) for t in low["htables"]]
    words = [len(data), len(low["htables"]), blocks, len(forms)]
    blob = np.frombuffer(data + b"\0" * (-len(data) % 4), dtype=np.int32)
    body, expect = [], []
    tabs, sel = [lists[t] for t in sets[:4]], int(sets[4])
    # the undamaged segments, decoded once with the reader's state at every MCU: a variant is decoded from the last state whose fetched bytes it shares
    whole, arr0 = {}, np.frombuffer(data, dtype=np.uint8)
    for first, count, begin, end in JD.split_segments(arr0, JD.find_markers(arr0), h["scan"], len(data), mcus, h["restart"])[0]:
        part, trace = np.zeros((count * per, 64), dtype=np.int16), []
        assert JD.entropy_decode_host(data, begin, end, tabs, sel, per, luma, count, part, 0, trace=trace) == 0
        whole[first, count] = (np.frombuffer(JD.clean_segment(data[begin:end]), dtype=np.uint8), part, trace, [t[1] for t in trace])
    cache = {}
    for length, edits in forms:
        b = bytearray(data[:length])
        for pos, val in edits:
            b[pos] = val
        b = bytes(b)
        arr = np.frombuffer(b, dtype=np.uint8)
        rows, _ = JD.split_segments(arr, JD.find_markers(arr), h["scan"], length, mcus, h["restart"])
        assert len(rows) == (1 if not h["restart"] else -(-mcus // h["restart"]))
        body += [length, len(edits), len(rows)] + [v for e in edits for v in e]
        coef = np.zeros((blocks, 64), dtype=np.int16)
        sts = []
        for first, count, begin, end in rows:
            assert 0 <= begin <= end <= length and first + count <= mcus
            body += [first * per, count, begin, end, per, luma, sel] + [int(t) for t in sets[:4]]
            key = (b[begin:end], first, count)                                  # a segment's decode is a pure function of its bytes and MCU range
            if key not in cache:
                clean0, part0, trace, fetched = whole[first, count]
                clean = np.frombuffer(JD.clean_segment(b[begin:end]), dtype=np.uint8)
                n = min(clean.size, clean0.size)
                differ = np.flatnonzero(clean[:n] != clean0[:n])
                shared = int(differ[0]) if differ.size else n                    # the reader's bytes agree up to here
                state = trace[max(bisect.bisect_right(fetched, shared) - 1, 0)]
                part = part0.copy()
                part[state[0] * per:] = 0
                cache[key] = (JD.entropy_decode_host(b, begin, end, tabs, sel, per, luma, count, part, 0, resume=state), part)
            st, part = cache[key]
            coef[first * per:(first + count) * per] = part
            sts.append(st)
        expect.append((sts, checksum(coef)))
    path = os.path.join(tmp, name + ".bin")
    with open(path, "wb") as f:
        f.write(np.array(words, dtype=np.int32).tobytes() + blob.tobytes() + low["htables"].astype(np.uint32).tobytes() + np.array(body, dtype=np.int32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, "the sanitized segment decoder did not exit clean on %s:\n%s" % (name, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(forms)
    for form, line, (sts, h64) in zip(forms, lines, expect):
        got = line.split()
        assert [int(v) for v in got[:-1]] == sts and got[-1] == h64, (name, form, line, sts, h64)
    return [(form, sts) for form, (sts, _) in zip(forms, expect)]


@pytest.mark.parametrize("name", NAMES)
def test_damaged_streams_under_the_sanitizers(sanitized, tmp_path, name):
    data = file_of(name)
    scan = JD.parse_header(data)["scan"]
    forms = [(len(data), ())] + damaged_forms(data, scan, np.random.default_rng(200))
    results = run_forms(sanitized, str(tmp_path), name, forms)
    assert results[0][1] == [0] * len(results[0][1])                            # the undamaged file
    seen = 0
    for _, sts in results[1:]:
        for s in sts:
            seen |= s
    assert seen & JD.ST_OVERRUN and results[-1][1][0] == JD.ST_BAD_CODE          # truncations overrun; the made vector's first segment has no code


def gpu_vectors():
    """the handful of damaged vectors the GPU test runs, all of which the sanitized program has passed above (they are forms of
    ``damaged_forms``): the 17 x 23 file truncated at three points of its scan, and the one that ends in BAD_CODE"""
    data = file_of("std_420_q75_17x23")
    scan = JD.parse_header(data)["scan"]
    bad = bytearray(data)
    for pos, val in bad_code_edits(scan):
        bad[pos] = val
    return [data[:scan + 1], data[:(scan + len(data)) // 2], data[:len(data) - 3], bytes(bad)]


def test_gpu_vectors_are_damaged_and_defined():
    vectors = gpu_vectors()
    frames, status = JD.decode_jpeg_host(vectors)
    assert status.tolist()[:3] == [JD.ST_OVERRUN] * 3 and status[3] == JD.ST_BAD_CODE
    assert all(f.shape == (17, 23, 3) for f in frames)
    assert not np.array_equal(frames[2], fixture()["rgb_std_420_q75_17x23"])
