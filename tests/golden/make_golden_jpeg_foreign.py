"""Mints tests/golden/jpeg_foreign.npz: baseline JPEG files as neither Pillow nor the project's own encoder writes them, and the pixels
Pillow 12 / libjpeg-turbo reads back from them -- ``Image.open(f).convert('RGB')``, or ``.convert('L')`` for the greyscale files.

    python tests/golden/make_golden_jpeg_foreign.py

The files come from tests/jpeg_writer.py: the STRUCTURE files are lossless rewrites of files Pillow wrote (the header rearranged around the
untouched scan bytes; their pixels must be Pillow's of the original, asserted here), the ENTROPY files are written whole with made Huffman
tables, selectors, extreme samples and given coefficients.  Keys: ``names``; ``origins``, per name the Pillow-written file it rewrites ("" for
none; the originals are in the set themselves, as ``pil_*``); per name ``file_<name>`` (uint8, the file's bytes), ``rgb_<name>`` (H,W,3) and,
for a greyscale file, ``l_<name>`` (H,W).  Written with fixed zip dates: the same script gives the same bytes."""
import io
import os
import sys
import zipfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_writer as JW  # noqa: E402
from make_golden_jpeg_decode import noise, save, smooth  # noqa: E402

LIMIT = 200 * 1024


def structure(rng):
    """(name, origin, bytes): files Pillow wrote, and their rewrites"""
    pil = {"pil_444_17x23": save(smooth(rng, 17, 23), quality=80, subsampling=0),
           "pil_420_37x45": save(smooth(rng, 37, 45), quality=75),
           "pil_420_rst2_25x40": save(smooth(rng, 25, 40), quality=85, restart_marker_blocks=2),
           "pil_grey_21x19": save(smooth(rng, 21, 19, 1), quality=75)}
    out = [(k, "", v) for k, v in pil.items()]
    m444, m420, mrst, mgrey = (JW.parse(pil[k]) for k in pil)
    assert all(JW.serialize(JW.parse(v)) == v for v in pil.values()), "parse / serialize is not lossless on Pillow's own layout"

    def add(name, origin, m, layout=None, **kw):
        out.append((name, origin, JW.serialize(m, layout, **kw)))

    def layout(m, jfif=True, first=(), dqt=None, dht=None, sof_first=False, before_sos=()):
        dqt = dqt if dqt is not None else [("DQT", [i]) for i in sorted(m["qt"])]
        dht = dht if dht is not None else [("DHT", [k]) for k in sorted(m["ht"], key=lambda k: (k[1], k[0]))]
        mid = [("SOF",)] + dqt + dht if sof_first else dqt + [("SOF",)] + dht
        return ([("JFIF",)] if jfif else []) + list(first) + mid + list(before_sos) + [("SOS",)]

    swapped = dict(m420, ht={(tc, 1 - th): t for (tc, th), t in m420["ht"].items()}, sel=[(1 - td, 1 - ta) for td, ta in m420["sel"]])
    add("swap_huffman_ids_420", "pil_420_37x45", swapped)
    add("merged_tables_444", "pil_444_17x23", m444, layout(m444, dqt=[("DQT", [0, 1])], dht=[("DHT", [(0, 0), (1, 0), (0, 1), (1, 1)])]))
    add("dri_before_sof_420", "pil_420_rst2_25x40", mrst, layout(mrst, first=[("DRI",)]))
    add("sof_before_tables_420", "pil_420_37x45", m420, layout(m420, sof_first=True))
    ids = lambda m, v: dict(m, comps=[(i,) + c[1:] for i, c in zip(v, m["comps"])])  # noqa: E731
    add("ids_0_1_2_nojfif_444", "pil_444_17x23", ids(m444, (0, 1, 2)), layout(m444, jfif=False))
    add("ids_10_20_30_nojfif_420", "pil_420_37x45", ids(m420, (10, 20, 30)), layout(m420, jfif=False))
    add("adobe_transform1_444", "pil_444_17x23", m444, layout(m444, jfif=False, first=[("ADOBE", 1)]))
    add("adobe_transform2_420", "pil_420_37x45", m420, layout(m420, jfif=False, first=[("ADOBE", 2)]))
    qswap = dict(m420, qt={1: m420["qt"][0], 0: m420["qt"][1]}, comps=[c[:3] + (1 - c[3],) for c in m420["comps"]])
    add("swap_quant_ids_420", "pil_420_37x45", qswap)
    third = [min(255, 2 * v + (k % 3)) for k, v in enumerate(m444["qt"][1])]                  # a third table, Cr's: other pixels than the original's
    add("three_quant_tables_444", "", dict(m444, qt={**m444["qt"], 2: third}, comps=m444["comps"][:2] + [m444["comps"][2][:3] + (2,)]))
    add("redefined_tables_420", "pil_420_37x45", m420,
        layout(m420, first=[("DQT", [(0, [7] * 64), (1, m420["qt"][0])]), ("DHT", [((1, 0), m420["ht"][1, 1]), ((0, 1), m420["ht"][0, 0])])]))
    for s in (0x22, 0x44):
        add("grey_sampling_%02x" % s, "pil_grey_21x19", dict(mgrey, comps=[(mgrey["comps"][0][0], s >> 4, s & 15, mgrey["comps"][0][3])]))
    add("fill_before_rst_and_eoi_420", "pil_420_rst2_25x40", mrst, layout(mrst, before_sos=[("DRI",)]), fill_rst=3, fill_eoi=3)
    bodies = b"a comment \xff\xd9 with \xff\xda markers \xff\xc2 in it \xff\xd8\xff"
    add("markers_in_com_app1_444", "pil_444_17x23", m444, layout(m444, first=[("COM", bodies), ("APP", 1, b"Exif\0\0" + bodies)], before_sos=[("COM", bodies[::-1])]))
    add("dri_0_444", "pil_444_17x23", m444, layout(m444, before_sos=[("DRI", 0)]))
    add("dri_65535_420", "pil_420_37x45", dict(m420, restart=65535), layout(m420, before_sos=[("DRI", 65535)]))
    return out, m444["qt"]


def entropy(rng, qt):
    """(name, "", bytes): files written whole"""
    out = []
    DC, AC = JW.DC_SYMBOLS, JW.AC_SYMBOLS
    flat = {(0, 0): JW.flat_table(DC), (1, 0): JW.flat_table(AC), (0, 1): JW.table(DC[::-1], 5), (1, 1): JW.table(AC[::-1], 9)}
    std = [(0, 0), (1, 1), (1, 1)]
    ones = {0: [1] * 64, 1: [1] * 64}
    coarse = {k: [min(255, 3 * v) for v in t] for k, t in qt.items()}

    def add(name, m, **kw):
        out.append((name, "", JW.serialize(m, **kw)))

    # (a) long codes: every DC code has 10 bits (table 0) or 16 (table 1), every AC code 15 or 16
    long_ = {(0, 0): JW.table(DC, 10), (0, 1): JW.table(DC, 16), (1, 0): JW.split_table(AC, 15, 16), (1, 1): JW.table(AC[::-1], 16)}
    add("long_codes_444_17x23", JW.from_image(noise(rng, 17, 23), "4:4:4", qt, long_, std))
    # (b) ladders: lengths 1 to 8 once each and the rest at 16; lengths 9 and 10, the look-ahead boundary
    ladder = {(0, 0): JW.ladder_table(DC[8:] + DC[:8]), (1, 0): JW.ladder_table(AC), (0, 1): JW.split_table(DC[::-1], 9, 10), (1, 1): JW.split_table(AC[::-1], 9, 10)}
    add("ladder_tables_420_23x17", JW.from_image(noise(rng, 23, 17), "4:2:0", qt, ladder, std))
    # (c) selectors
    add("sel_y10_cb01_cr10_444_9x17", JW.from_image(noise(rng, 9, 17), "4:4:4", qt, flat, [(1, 0), (0, 1), (1, 0)]))
    add("sel_all_00_two_tables_444_9x9", JW.from_image(noise(rng, 9, 9), "4:4:4", qt, {k: flat[k] for k in ((0, 0), (1, 0))}, [(0, 0)] * 3))
    add("sel_all_10_rst3_420_33x31", JW.from_image(smooth(rng, 33, 31), "4:2:0", qt, {(0, 1): ladder[0, 1], (1, 0): flat[1, 0]}, [(1, 0)] * 3, restart=3))
    add("sel_grey_11_13x9", JW.from_image(noise(rng, 13, 9, 1), "L", qt, {(0, 1): flat[0, 1], (1, 1): flat[1, 1]}, [(1, 1)]))
    # (d) extremes from real samples, quantisation tables of all ones
    board = np.kron(np.indices((2, 4)).sum(axis=0) % 2, np.ones((8, 8))).astype(np.uint8) * 255            # flat 8 x 8 blocks, 0 and 255 alternating
    add("dc_category_11_grey_16x32", JW.from_image(board, "L", ones, flat, [(0, 0)]))
    board = np.kron(np.indices((4, 4)).sum(axis=0) % 2, np.ones((8, 8))).astype(np.uint8) * 255
    add("dc_category_11_rst1_420_32x32", JW.from_image(np.repeat(board[:, :, None], 3, axis=2), "4:2:0", ones, flat, [(0, 0), (0, 0), (1, 1)], restart=1))
    pixels = (np.indices((8, 16)).sum(axis=0) + (np.arange(16) >= 8)) % 2 * 255                              # a one-pixel checkerboard, its phase flipped in the second block
    add("ac_size_10_at_63_grey_8x16", JW.from_image(pixels.astype(np.uint8), "L", ones, flat, [(0, 0)]))
    # (e) runs, as given coefficients
    blocks = np.zeros((6, 64), dtype=np.int16)
    blocks[0, 63] = 37                                                                                       # ZRL x 3, then run 14
    blocks[1, 0], blocks[1, 63] = 40, -37
    blocks[2, 1:] = [(1 + k % 2) * (-1) ** (k // 2) for k in range(63)]                                      # all 63 ACs: no EOB
    blocks[4, 0] = -25                                                                                       # blocks 3 and 4: an EOB alone
    blocks[5, 16], blocks[5, 48] = 5, -3                                                                     # run 15 with a size, ZRL, run 15 with a size
    add("runs_grey_16x24", JW.from_coefficients(blocks, 16, 24, "L", ones, flat, [(0, 0)]))
    # (f) many segments: 60 intervals of one MCU, 3 3/4 workgroups of them, RST0..7 seven times round
    many = {(0, 0): flat[0, 0], (0, 1): ladder[0, 0], (1, 0): ladder[1, 1], (1, 1): flat[1, 0]}
    add("rst1_60_segments_444_48x80", JW.from_image(noise(rng, 48, 80), "4:4:4", coarse, many, [(0, 1), (1, 0), (0, 0)], restart=1))
    return out


def pixels(out, name, data):
    im = Image.open(io.BytesIO(data))
    out["file_" + name] = np.frombuffer(data, dtype=np.uint8)
    out["rgb_" + name] = np.asarray(im.convert("RGB"))
    if im.mode == "L":
        out["l_" + name] = np.asarray(im.convert("L"))


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    rng = np.random.default_rng(20261020)
    files, qt = structure(rng)
    files += entropy(rng, qt)
    out = {"names": np.array([f[0] for f in files]), "origins": np.array([f[1] for f in files])}
    for name, origin, data in files:
        pixels(out, name, data)
        assert max(out["rgb_" + name].shape[:2]) <= 80 and min(out["rgb_" + name].shape[:2]) <= 48, name
        if origin:
            assert np.array_equal(out["rgb_" + name], out["rgb_" + origin]), "%s does not decode to its original's pixels" % name
    path = os.path.join(HERE, "jpeg_foreign.npz")
    save_npz(path, out)
    assert os.path.getsize(path) < LIMIT, "jpeg_foreign.npz has %d bytes, the limit is %d" % (os.path.getsize(path), LIMIT)
    print("jpeg_foreign.npz", os.path.getsize(path), "bytes,", len(files), "files")


if __name__ == "__main__":
    main()
