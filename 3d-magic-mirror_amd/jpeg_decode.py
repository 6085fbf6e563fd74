"""Baseline JPEG files as device frames, Pillow's pixels: host side of ``mm_jpeg_decode`` (csrc/mm_jpeg_decode.hip).

Every image the reference consumes is a JPEG file somebody else wrote: the datasets open ``JPEGImages/*.jpg`` per sample
(datasets/market.py, atr.py, atr2.py, bird.py) and the evaluation re-opens its ``ori`` / ``rec`` / ``inter`` directories one
``Image.open(f).convert('RGB')`` at a time (test.py:430-463, trainer.py:771-836, fid_score.py:71-76).  ``decode_jpeg`` takes the files'
bytes and leaves the frames in device memory, packed like ``ImagePool``: one upload (the concatenated bytes and the tables), one memset and
three launches whatever the number of files.  Every pixel equals Pillow 12's (libjpeg-turbo's islow IDCT, fancy upsampling, fixed-point
YCbCr -> RGB): integer arithmetic on both sides, compared without a tolerance.

    frames = decode_jpeg([open(p, "rb").read() for p in paths])        # or the paths themselves, or an encode_jpeg JpegBatch
    frames.frames[i]                                                   # (H_i, W_i, 3) uint8 view; frames.stack() when the sizes agree
    pool = ImagePool.from_jpeg(files, segs, device)                    # input_batches.py: decoded straight into the pool's buffer

Accepted: baseline sequential (SOF0), 8 bits, one interleaved scan; three components YCbCr with luma 2x2, 2x1 or 1x1 and chroma 1x1, or one
component (any sampling factor, treated as 1x1); any 8-bit DQT; any valid DHT with ids 0 / 1 (so ``optimize=True`` files); DRI with any
interval; APPn / COM skipped; fill bytes before markers; bytes after EOI ignored, a missing EOI tolerated.
Rejected by the parser (ValueError naming the file's index; nothing is launched): progressive / extended / lossless / arithmetic frames
(SOF1 and above), 12-bit samples, 16-bit DQT, more than one scan, DNL, 4:1:1 / 4:4:0 and other samplings, 2 or 4 components, RGB files (an
Adobe marker with transform 0, or component ids R, G, B), a scan that names a table the file never defined, a segment length that runs
past the file, no SOI / SOF / SOS.
Damaged entropy-coded data is not an error of the parser: the kernel cannot read or write out of range for any bytes, a damaged segment
stops at the damage with the rest of its coefficients zero, and the file's ``status`` gets ST_OVERRUN / ST_BAD_CODE / ST_BAD_RUN /
ST_BAD_SIZE.  Such a file's pixels are defined by ``decode_jpeg_host``, not by Pillow (which raises, or conceals differently).

Out of scope: progressive and arithmetic coding, 12-bit, CMYK / YCCK, non-interleaved scans, 4:1:1 and 4:4:0, reading directories,
anything differentiable.  PNG files (the datasets' masks) are ``decode_png``'s, in png_decode.py."""
import os
import re

import numpy as np
import torch

from . import _native as N
from .jpeg import MAX_BLOCKS, MCU, MODES, ZIGZAG, JpegBatch, plane_bytes

ST_OVERRUN, ST_BAD_CODE, ST_BAD_RUN, ST_BAD_SIZE = 1, 2, 4, 8      # MM_JPEG_ST_* (csrc/mm_jpeg_entropy.h)
STATUS_NAMES = ((ST_OVERRUN, "OVERRUN"), (ST_BAD_CODE, "BAD_CODE"), (ST_BAD_RUN, "BAD_RUN"), (ST_BAD_SIZE, "BAD_SIZE"))
LAYOUTS = ("4:2:0", "4:2:2", "4:4:4", "L")                          # a file record's layout word indexes this
SHAPES = tuple((per, lh * lv, 8 * lh, 8 * lv) for per, lh, lv, _ in (MCU[k] for k in LAYOUTS))      # per layout: blocks per MCU, luma blocks of them, MCU width, MCU height
FILE_INTS, SEGMENT_INTS, SET_INTS, TABLE_WORDS = N.JPEG_DEC_FILE_INTS, N.JPEG_DEC_SEGMENT_INTS, N.JPEG_DEC_SET_INTS, N.JPEG_TABLE_WORDS
(F_H, F_W, F_LAYOUT, F_MX, F_MY, F_BLOCK0, F_YOFF, F_COFF, F_Q0) = range(9)
(S_FILE, S_FIRST, S_COUNT, S_BEGIN, S_END, S_SET) = range(6)
GROUP = N.JPEG_DEC_GROUP                                            # segments of one workgroup: they share a table set


def _fail(i, why):
    raise ValueError("file %d: %s" % (i, why))


def huffman_decode_table(bits, vals):
    """One DHT table (16 counts, the symbols) as the TABLE_WORDS uint32 words the decoder reads: 512 look-ahead entries of 16 bits
    (``length << 8 | symbol`` for codes of up to 9 bits, 0 for longer ones), libjpeg's maxcode[0..17] (-1: none of that length) and
    valoffset[0..17], and the 256 symbols.  None if the counts oversubscribe the code space."""
    look = np.zeros(512, dtype=np.uint16)
    maxcode = np.full(18, -1, dtype=np.int32)
    valoff = np.zeros(18, dtype=np.int32)
    syms = np.zeros(256, dtype=np.uint8)
    syms[:len(vals)] = np.frombuffer(bytes(vals), dtype=np.uint8)
    code = k = 0
    for length in range(1, 17):
        cnt = bits[length - 1]
        if cnt:
            if code + cnt > 1 << length:
                return None
            valoff[length] = k - code
            if length <= 9:
                for j in range(cnt):
                    look[(code + j) << (9 - length):(code + j + 1) << (9 - length)] = length << 8 | vals[k + j]
            code, k = code + cnt, k + cnt
            maxcode[length] = code - 1
        code <<= 1
    maxcode[17] = 0xFFFFF
    return np.concatenate([look.view(np.uint32), maxcode.view(np.uint32), valoff.view(np.uint32), syms.view(np.uint32)])


def parse_header(data, i=0):
    """The markers of one file up to and including SOS (host arithmetic): a dict of H, W, layout (an index of LAYOUTS), qtables (three tuples
    of 64, natural order, per component; a greyscale file repeats its one), huffman (per component its (DC, AC) tables as (counts, symbols)
    pairs of bytes), restart (MCUs per interval, 0: none) and scan, the index of the first entropy-coded byte.  ValueError for what is
    rejected, naming file ``i``."""
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        _fail(i, "no SOI marker: not a JPEG file")
    pos, qt, ht, frame, restart, adobe = 2, {}, {}, None, 0, None
    while True:
        if pos >= n:
            _fail(i, "no SOF marker" if frame is None else "no SOS marker")
        if data[pos] != 0xFF:
            _fail(i, "byte %d is 0x%02X where a marker must begin" % (pos, data[pos]))
        while pos < n and data[pos] == 0xFF:                          # fill bytes
            pos += 1
        if pos >= n:
            _fail(i, "no SOF marker" if frame is None else "no SOS marker")
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD8:                            # TEM, RSTn, SOI: no length
            continue
        if m == 0xD9:
            _fail(i, "no SOF marker" if frame is None else "no SOS marker")
        length = (data[pos] << 8 | data[pos + 1]) if pos + 2 <= n else 0
        if length < 2 or pos + length > n:
            _fail(i, "the length of segment 0x%02X at byte %d runs past the file" % (m, pos - 2))
        body = bytes(data[pos + 2:pos + length])
        pos += length
        if m == 0xC0:
            if frame is not None:
                _fail(i, "more than one frame")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                _fail(i, "a malformed SOF0 segment")
            if body[0] != 8:
                _fail(i, "%d-bit precision, only 8-bit samples are decoded" % body[0])
            frame = dict(H=body[1] << 8 | body[2], W=body[3] << 8 | body[4], comps=[(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(body[5])])
        elif m == 0xC2:
            _fail(i, "a progressive file (SOF2), only baseline is decoded")
        elif m in (0xC1, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xCC):
            _fail(i, "marker 0x%02X: an extended, lossless or arithmetic coding process, only baseline is decoded" % m)
        elif m == 0xDB:
            at = 0
            while at < len(body):
                if body[at] >> 4:
                    _fail(i, "a 16-bit DQT, only 8-bit tables are decoded")
                if (body[at] & 15) > 3 or at + 65 > len(body):
                    _fail(i, "a malformed DQT segment")
                t = np.zeros(64, dtype=np.int32)
                t[ZIGZAG] = np.frombuffer(body, dtype=np.uint8, count=64, offset=at + 1)
                if t.min() < 1:
                    _fail(i, "a quantisation table with a zero entry")
                qt[body[at] & 15] = tuple(int(v) for v in t)
                at += 65
        elif m == 0xC4:
            at = 0
            while at < len(body):
                if at + 17 > len(body):
                    _fail(i, "a malformed DHT segment")
                tc, th, bits = body[at] >> 4, body[at] & 15, body[at + 1:at + 17]
                count = sum(bits)
                if tc > 1 or th > 1:
                    _fail(i, "Huffman table class %d id %d, only classes and ids 0 / 1 are decoded" % (tc, th))
                if count > 256 or at + 17 + count > len(body):
                    _fail(i, "a malformed DHT segment")
                ht[tc, th] = (bits, body[at + 17:at + 17 + count])
                at += 17 + count
        elif m == 0xDD:
            if len(body) != 2:
                _fail(i, "a malformed DRI segment")
            restart = body[0] << 8 | body[1]
        elif m == 0xDC:
            _fail(i, "a DNL marker")
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xDA:
            break
    if frame is None:
        _fail(i, "no SOF marker before SOS")
    H, W, comps = frame["H"], frame["W"], frame["comps"]
    if H == 0:
        _fail(i, "a height of 0 (to come from a DNL marker)")
    if W == 0:
        _fail(i, "a width of 0")
    if len(comps) not in (1, 3):
        _fail(i, "%d components, only 1 (greyscale) and 3 (YCbCr) are decoded" % len(comps))
    if len(comps) == 3:
        if adobe == 0 or tuple(c[0] for c in comps) == (0x52, 0x47, 0x42):
            _fail(i, "an RGB file (%s), only YCbCr is decoded" % ("Adobe transform 0" if adobe == 0 else "component ids R, G, B"))
        luma = comps[0][1:3]
        if comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1) or luma not in ((2, 2), (2, 1), (1, 1)):
            _fail(i, "sampling %s, only 4:2:0, 4:2:2 and 4:4:4 are decoded (not 4:1:1, 4:4:0, ...)" % ", ".join("%dx%d" % c[1:3] for c in comps))
        layout = {(2, 2): 0, (2, 1): 1, (1, 1): 2}[luma]
    else:
        layout = 3
    if len(body) < 1 or len(body) != 4 + 2 * body[0]:
        _fail(i, "a malformed SOS segment")
    if body[0] != len(comps) or any(body[1 + 2 * c] != comps[c][0] for c in range(len(comps))):
        _fail(i, "a scan of %d of %d components: more than one scan (non-interleaved), only one interleaved scan is decoded" % (body[0], len(comps)))
    if tuple(body[-3:]) != (0, 63, 0):
        _fail(i, "a scan with spectral selection or successive approximation")
    huffman, qtables = [], []
    for c in range(len(comps)):
        td, ta = body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15
        if (0, td) not in ht or (1, ta) not in ht:
            _fail(i, "the scan names Huffman table %s %d, which the file never defined" % (("DC", td) if (0, td) not in ht else ("AC", ta)))
        if comps[c][3] not in qt:
            _fail(i, "the frame names quantisation table %d, which the file never defined" % comps[c][3])
        huffman.append((ht[0, td], ht[1, ta]))
        qtables.append(qt[comps[c][3]])
    per, _, mw, mh = SHAPES[layout]
    mx, my = (W + mw - 1) // mw, (H + mh - 1) // mh
    if mx * my * per > MAX_BLOCKS:
        _fail(i, "%d x %d has %d blocks, more than %d" % (H, W, mx * my * per, MAX_BLOCKS))
    return dict(H=H, W=W, layout=layout, mx=mx, my=my, qtables=(qtables * 3)[:3], huffman=(huffman * 3)[:3], restart=restart, scan=pos)


def find_markers(data):
    """the indices i of a uint8 array where a marker begins: data[i] == 0xFF and data[i + 1] is neither 0x00 (stuffing) nor 0xFF (i is a
    fill byte then).  One vectorised pass."""
    return np.flatnonzero((data[:-1] == 0xFF) & (data[1:] != 0) & (data[1:] != 0xFF))


def split_segments(data, markers, scan, end, mcus, restart):
    """The restart intervals of one scan, data[scan:end], as (first MCU, MCU count, byte begin, byte end) rows, and the marker byte that ended
    the scan (None: the file's end).  ``markers``: ``find_markers`` of data (any superset of this scan's).  FF D0..D7 close an interval;
    the first other marker ends the scan.  There are ceil(mcus / restart) rows whatever the bytes hold: intervals the scan does not have
    are empty (their decode overruns at once), markers beyond the last expected interval are ignored."""
    want = 1 if restart == 0 else (mcus + restart - 1) // restart
    step = mcus if restart == 0 else restart
    rows, begin, ended = [], scan, None
    a, b = np.searchsorted(markers, [scan, end - 1])
    for m in markers[a:b].tolist():
        code = int(data[m + 1])
        if 0xD0 <= code <= 0xD7 and len(rows) < want - 1:
            rows.append((len(rows) * step, step, begin, m))
            begin = m + 2
        elif not 0xD0 <= code <= 0xD7:
            ended, end = code, m
            break
    while len(rows) < want:
        first = len(rows) * step
        rows.append((first, min(step, mcus - first), begin, end))
        begin = end
    return rows, ended


def _read(f, i):
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    if isinstance(f, (str, os.PathLike)):
        with open(f, "rb") as h:
            return h.read()
    raise ValueError("file %d: need bytes, a bytearray or a path, got %s" % (i, type(f)))


def lower_jpeg_decode(files, mode="RGB"):
    """Files as the tables ``mm_jpeg_decode`` reads (host arithmetic only, no device; MMJpegDecodeDesc in include/mm_render.h has the
    layouts): a dict of n; mode; data, the files back to back (uint8); starts (n + 1), where each begins in it; files (n, 16) int32, the
    per-file records; offsets (n + 1) int64 and sizes (n, 2) int32 rows (H, W), the packing of the output; segments (S, 6) int32 rows
    {file, first MCU, MCU count, byte begin, byte end, table set}, grouped by table set, each group padded with count-0 rows to a multiple
    of GROUP; qtables (Q, 64) int32, natural order, and htables (T, 356) uint32, each deduplicated over the batch; sets (K, 8) int32 rows
    {DC 0, DC 1, AC 0, AC 1, selector bits}; tables, all of these as the one int32 array the library takes; blocks, plane_bytes, channels,
    status_offset and workspace_bytes (mm_jpeg_decode_query_workspace in Python).  ValueError, naming the file's index and the reason, for
    everything the parser rejects."""
    if mode not in MODES:
        raise ValueError("mode must be 'RGB' or 'L', got %r" % (mode,))
    if isinstance(files, JpegBatch):
        raw = np.frombuffer(files._view, dtype=np.uint8)
        starts = np.asarray(files.offsets, dtype=np.int64)
        data = raw[:int(starts[-1])]
        if starts[0] != 0 or len(starts) < 2:
            raise ValueError("an empty JpegBatch")
    else:
        blobs = [_read(f, i) for i, f in enumerate(files)]
        if not blobs:
            raise ValueError("an empty list of files")
        starts = np.zeros(len(blobs) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in blobs], out=starts[1:])
        data = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    n = len(starts) - 1
    if n > N.JPEG_DEC_MAX_FILES or data.size >= 1 << 31:
        raise ValueError("%d files of %d bytes: at most %d files and 2^31 - 1 bytes in a call" % (n, data.size, N.JPEG_DEC_MAX_FILES))
    markers = find_markers(data) if data.size > 1 else np.zeros(0, dtype=np.int64)
    view = memoryview(data)
    recs = np.zeros((n, FILE_INTS), dtype=np.int32)
    qindex, hindex, sindex, htables, segments = {}, {}, {}, [], []
    block0 = plane = 0
    head = h = None
    for i in range(n):
        a, b = int(starts[i]), int(starts[i + 1])
        if head is None or b - a < len(head) or view[a:a + len(head)] != head:   # (a dataset repeats one header: the same bytes parse to the same dict)
            h = parse_header(view[a:b], i)
            head = bytes(view[a:a + h["scan"]])
        if mode == "L" and h["layout"] != 3:
            _fail(i, "a colour file with mode 'L' (mode 'L' decodes greyscale files only; Pillow's RGB -> L formula is not part of this)")
        mcus = h["mx"] * h["my"]
        rows, ended = split_segments(data, markers, a + h["scan"], b, mcus, h["restart"])
        if ended in (0xDA, 0xC4, 0xDB, 0xDD):
            _fail(i, "more than one scan")
        if ended == 0xDC:
            _fail(i, "a DNL marker")
        hts = []
        for dc_ac in h["huffman"]:
            for t in dc_ac:
                if t not in hindex:
                    words = huffman_decode_table(*t)
                    if words is None:
                        _fail(i, "a DHT segment whose counts oversubscribe the code space")
                    hindex[t] = len(htables)
                    htables.append(words)
                hts.append(hindex[t])
        dcs, acs = sorted(set(hts[0::2])), sorted(set(hts[1::2]))              # (at most two of each: the ids are 0 / 1)
        key = (dcs[0], dcs[-1], acs[0], acs[-1], sum((dcs.index(hts[2 * c]) << 2 * c) | (acs.index(hts[2 * c + 1]) << (2 * c + 1)) for c in range(3)))
        s = sindex.setdefault(key, len(sindex))
        segments.extend((s, i) + r for r in rows)
        q = [qindex.setdefault(t, len(qindex)) for t in h["qtables"]]
        luma, chroma = plane_bytes(LAYOUTS[h["layout"]], mcus)
        recs[i, :F_Q0 + 3] = (h["H"], h["W"], h["layout"], h["mx"], h["my"], block0, plane, plane + luma if chroma else 0, q[0], q[1], q[2])
        block0, plane = block0 + mcus * SHAPES[h["layout"]][0], plane + luma + chroma
        if block0 > N.JPEG_DEC_MAX_BLOCKS:
            raise ValueError("files 0..%d have %d blocks, more than %d in a call" % (i, block0, N.JPEG_DEC_MAX_BLOCKS))
    sizes = recs[:, :2].copy()
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(sizes[:, 0].astype(np.int64) * sizes[:, 1], out=offsets[1:])
    segments.sort(key=lambda r: r[0])                                           # stable: by table set, then in input order
    arr = np.array(segments, dtype=np.int64).reshape(-1, 6)
    parts = []
    for s in range(len(sindex)):
        rows = arr[arr[:, 0] == s]
        part = np.zeros(((len(rows) + GROUP - 1) // GROUP * GROUP, SEGMENT_INTS), dtype=np.int32)
        part[:, S_SET] = s
        part[:len(rows), :S_SET] = rows[:, 1:]
        parts.append(part)
    seg = np.concatenate(parts)
    qtables = np.array(sorted(qindex, key=qindex.get), dtype=np.int32).reshape(-1, 64)
    htab = np.stack(htables).astype(np.uint32)
    sets = np.zeros((len(sindex), SET_INTS), dtype=np.int32)
    sets[:, :5] = np.array(sorted(sindex, key=sindex.get), dtype=np.int32).reshape(-1, 5)
    tables = np.concatenate([recs.reshape(-1), offsets.view(np.int32), seg.reshape(-1), qtables.reshape(-1), htab.view(np.int32).reshape(-1), sets.reshape(-1)])
    status_offset = N.up256(block0 * 128)
    return dict(n=n, mode=mode, channels=3 if mode == "RGB" else 1, data=data, starts=starts, files=recs, offsets=offsets, sizes=sizes, segments=seg,
                qtables=qtables, htables=htab, sets=sets, tables=tables, blocks=block0, plane_bytes=plane, status_offset=status_offset,
                workspace_bytes=status_offset + N.up256(4 * n) + N.up256(plane))


# ---- the decoder restated on the host, in the kernel's order ----------------------------------------------------------------------------
_STOP = re.compile(b"\xff+(?:[^\x00\xff]|\\Z)", re.DOTALL)       # where the bit reader stops: FFs followed by neither 00 nor FF, or by the end
_STUFFED = re.compile(b"\xff+\x00", re.DOTALL)                    # fill bytes and a stuffed FF: one data FF


def clean_segment(seg):
    """what the bit reader sees of a segment's bytes: everything from the stop on (FFs followed by neither 00 nor FF, or by the end) cut off,
    fill bytes and stuffing removed"""
    m = _STOP.search(seg)
    return _STUFFED.sub(b"\xff", seg[:m.start()] if m else seg)


def entropy_decode_host(raw, begin, end, tables, sel, per, luma, count, coef, block0, trace=None, resume=None):
    """``jpeg_decode_segment`` of csrc/mm_jpeg_entropy.h in Python: ``count`` MCUs of ``per`` blocks from raw[begin:end] (bytes) into
    rows block0.. of ``coef`` (blocks, 64) int16, zigzag order, zeroed before.  tables: the four tables of the set as (look, maxcode, valoff,
    symbols) lists (``_table_lists``).  Returns the segment's status.
    trace: a list that receives the reader's state at every MCU's start, (MCU, bytes fetched, unread bits, accumulator, predictors);
    resume: one such state to go on from -- valid for any segment whose ``clean_segment`` agrees with the traced one's over the bytes
    fetched (the damaged-stream tests decode thousands of variants of one segment this way; the rows before that MCU are the caller's)."""
    clean = clean_segment(raw[begin:end])
    avail = 8 * len(clean)                                          # consuming more than these is an overrun: the reader supplies zeros
    clean += b"\0" * 16
    pos = acc = nb = start = 0
    preds = [0, 0, 0]
    if resume is not None:
        start, pos, nb, acc = resume[:4]
        preds = list(resume[4])
    for mcu in range(start, count):
        if trace is not None:
            trace.append((mcu, pos, nb, acc, tuple(preds)))
        for j in range(per):
            c = 0 if j < luma else j - luma + 1
            row = coef[block0 + mcu * per + j]
            k = 0
            while k < 64:
                look, maxcode, valoff, syms = tables[(sel >> 2 * c) & 1] if k == 0 else tables[2 + ((sel >> (2 * c + 1)) & 1)]
                if nb < 32:
                    acc = ((acc & ((1 << nb) - 1)) << 32) | int.from_bytes(clean[pos:pos + 4].ljust(4, b"\0"), "big")
                    pos += 4
                    nb += 32
                peek = (acc >> (nb - 16)) & 0xFFFF
                e = look[peek >> 7]
                if e:
                    nb -= e >> 8
                    sym = e & 255
                else:
                    for length in range(10, 17):
                        code = peek >> (16 - length)
                        if code <= maxcode[length]:
                            sym = syms[(code + valoff[length]) & 255]
                            nb -= length
                            break
                    else:
                        return ST_BAD_CODE
                if k == 0:
                    s = sym
                    if s > 11:
                        return ST_BAD_SIZE
                    r = 0
                else:
                    r, s = sym >> 4, sym & 15
                    if s == 0:
                        if 8 * pos - nb > avail:
                            return ST_OVERRUN
                        if r != 15:
                            break
                        if k + 16 > 64:
                            return ST_BAD_RUN
                        k += 16
                        continue
                    if s > 10:
                        return ST_BAD_SIZE
                    k += r
                    if k > 63:
                        return ST_BAD_RUN
                v = 0
                if s:
                    nb -= s
                    v = (acc >> nb) & ((1 << s) - 1)
                    if v < 1 << (s - 1):
                        v -= (1 << s) - 1
                if 8 * pos - nb > avail:
                    return ST_OVERRUN
                if k == 0:
                    v = preds[c] = ((preds[c] + v + 32768) & 0xFFFF) - 32768
                    if v:
                        row[0] = v
                else:
                    row[k] = v
                k += 1
    return 0


def _table_lists(words):
    look = words[:256].view(np.uint16).tolist()
    return (look, words[256:274].view(np.int32).tolist(), words[274:292].view(np.int32).tolist(), words[292:356].view(np.uint8).tolist())


def coefficients_host(low):
    """the entropy decode of every segment of ``lower_jpeg_decode``'s dict: (coef (blocks, 64) int16 in zigzag order, status (n) int32)"""
    coef = np.zeros((low["blocks"], 64), dtype=np.int16)
    status = np.zeros(low["n"], dtype=np.int32)
    raw = low["data"].tobytes()
    lists = [_table_lists(t) for t in low["htables"]]
    for f, first, count, begin, end, s in low["segments"].tolist():
        if count == 0:
            continue
        per, luma = SHAPES[low["files"][f, F_LAYOUT]][:2]
        st = low["sets"][s]
        status[f] |= entropy_decode_host(raw, begin, end, [lists[t] for t in st[:4]], int(st[4]), per, luma, count, coef, int(low["files"][f, F_BLOCK0]) + first * per)
    return coef, status


def _idct8(i, bits):
    """``jpeg_idct8`` of csrc/mm_jpeg_idct.h over int32 arrays (wrapping like the registers do)"""
    R = 1 << (bits - 1)
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) * (1 << 13), (i[0] - i[4]) * (1 << 13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + (z1 + z3), a1 + (z2 + z4), a2 + (z2 + z3), a3 + (z1 + z4)
    return [(t10 + a3 + R) >> bits, (t11 + a2 + R) >> bits, (t12 + a1 + R) >> bits, (t13 + a0 + R) >> bits,
            (t13 - a0 + R) >> bits, (t12 - a1 + R) >> bits, (t11 - a2 + R) >> bits, (t10 - a3 + R) >> bits]


def idct_blocks_host(coef, q):
    """(B, 64) int16 zigzag blocks, dequantised by q (64, natural order), through the islow IDCT: (B, 8, 8) uint8 samples"""
    nat = np.zeros(coef.shape, dtype=np.int32)
    nat[:, ZIGZAG] = coef
    d = (nat * np.asarray(q, dtype=np.int32)).reshape(-1, 8, 8)
    with np.errstate(over="ignore"):
        cols = _idct8([d[:, k, :] for k in range(8)], 11)            # the column pass: cols[k] is row k of the workspace
        ws = np.stack(cols, axis=1)
        rows = _idct8([ws[:, :, c] for c in range(8)], 18)
    return np.clip(np.stack(rows, axis=2) + 128, 0, 255).astype(np.uint8)


def _plane(blocks, rows, cols):
    """(rows * cols, 8, 8) blocks in raster order as one (8 rows, 8 cols) plane"""
    return blocks.reshape(rows, cols, 8, 8).transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)


def _upsample(c, layout, H, W):
    """``jpeg_chroma_up_at``: a padded chroma plane as (H, W) int32"""
    c = c.astype(np.int32)
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    hd, wd = (H + 1) // 2, (W + 1) // 2
    if layout == 2:
        return c[:H, :W]
    cx = x >> 1
    ox = np.where(x & 1, np.minimum(cx + 1, wd - 1), np.maximum(cx - 1, 0))
    if layout == 1:
        if wd <= 2:
            return c[y, cx]
        return (3 * c[y, cx] + c[y, ox] + np.where(x & 1, 2, 1)) >> 2
    r = y >> 1
    if wd <= 2:
        return c[r, cx]
    qr = np.where(y & 1, np.minimum(r + 1, hd - 1), np.maximum(r - 1, 0))
    s, so = 3 * c[r, cx] + c[qr, cx], 3 * c[r, ox] + c[qr, ox]
    return (3 * s + so + np.where(x & 1, 7, 8)) >> 4


def pixels_host(low, coef):
    """coefficients to frames, per file: dequantise, IDCT, upsample, convert -- the arithmetic of the idct and pixels kernels"""
    frames = []
    for i in range(low["n"]):
        rec = low["files"][i]
        H, W, layout, mx, my, block0 = (int(v) for v in rec[:6])
        per, luma, mw, mh = SHAPES[layout]
        blk = coef[block0:block0 + mx * my * per].reshape(my, mx, per, 64)
        q = [low["qtables"][rec[F_Q0 + c]] for c in range(3)]
        lv, lh = mh // 8, mw // 8
        yb = idct_blocks_host(blk[:, :, :luma].reshape(-1, 64), q[0]).reshape(my, mx, lv, lh, 8, 8)
        Y = yb.transpose(0, 2, 4, 1, 3, 5).reshape(my * mh, mx * mw)[:H, :W].astype(np.int32)
        if layout == 3:
            g = Y.astype(np.uint8)
            frames.append(np.repeat(g[:, :, None], 3, axis=2) if low["mode"] == "RGB" else g)
            continue
        cb, cr = (_upsample(_plane(idct_blocks_host(blk[:, :, luma + c].reshape(-1, 64), q[1 + c]), my, mx), layout, H, W) - 128 for c in range(2))
        rgb = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)], axis=2)
        frames.append(np.clip(rgb, 0, 255).astype(np.uint8))
    return frames


def decode_jpeg_host(files, mode="RGB"):
    """The whole decoder on the host, in numpy and Python, in the kernels' order: (frames, status) -- a list of (H_i, W_i, 3) uint8 arrays
    ((H_i, W_i) in mode "L") and the (n) int32 status words.  The yardstick where Pillow is not installed, and the definition of what a
    damaged file decodes to; tests/test_jpeg_decode_host.py holds it to Pillow."""
    low = lower_jpeg_decode(files, mode)
    coef, status = coefficients_host(low)
    return pixels_host(low, coef), status


# ---- the device path ----------------------------------------------------------------------------------------------------------------------
class DecodedFrames:
    """``decode_jpeg``'s result.  images: the packed uint8 device buffer, file i at pixel offsets[i] (byte 3 * offsets[i]; byte offsets[i]
    in mode "L"), no padding -- ``ImagePool``'s packing; offsets (n + 1) int64 and sizes (n, 2) int32 rows (H, W), host arrays; status (n)
    int32 on the device, 0 for a clean file, else ST_* bits; frames[i]: the (H_i, W_i, 3) view of file i ((H_i, W_i) in mode "L")."""

    def __init__(self, images, offsets, sizes, status, mode):
        self.images, self.offsets, self.sizes, self.status, self.mode = images, offsets, sizes, status, mode
        ch = {"RGB": 3, "RGBA": 4}.get(mode, 1)                           # ("RGBA": decode_png's)
        self.frames = [images[ch * int(offsets[i]):ch * int(offsets[i + 1])].view((int(h), int(w), ch) if ch > 1 else (int(h), int(w)))
                       for i, (h, w) in enumerate(sizes.tolist())]

    def __len__(self):
        return len(self.frames)

    def stack(self):
        """(n, H, W, 3) (or (n, H, W)) when all sizes agree -- a view, nothing is copied; ValueError otherwise"""
        if (self.sizes != self.sizes[0]).any():
            raise ValueError("the files have different sizes: %s" % sorted(set(map(tuple, self.sizes.tolist()))))
        return self.images.view((len(self),) + tuple(self.frames[0].shape))


def status_text(st):
    return "|".join(name for bit, name in STATUS_NAMES if st & bit) or "0"


def _upload(low, device):
    """one pinned host buffer -- the tables, then on a 16-byte boundary the files' bytes -- and its one copy to the device: (host, dev, where
    the bytes start)"""
    b0 = (4 * low["tables"].size + 15) // 16 * 16
    host = torch.empty(b0 + low["data"].size, dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    hv[:4 * low["tables"].size] = low["tables"].view(np.uint8)
    hv[b0:] = low["data"]
    return host, host.to(device, non_blocking=True), b0


def _launch(low, host, dev_buf, b0, out):
    """``mm_jpeg_decode`` of an uploaded batch into ``out`` on the current stream: the workspace (its status words at status_offset)"""
    d = N.MMJpegDecodeDesc()
    d.n, d.mode, d.n_segments = low["n"], MODES[low["mode"]], low["segments"].shape[0]
    d.n_qtables, d.n_htables, d.n_sets, d.n_bytes = low["qtables"].shape[0], low["htables"].shape[0], low["sets"].shape[0], low["data"].size
    d.bytes, d.tables_host, d.tables, d.out = dev_buf.data_ptr() + b0, host.data_ptr(), dev_buf.data_ptr(), N.ptr(out)
    ws = N.checked_workspace("mm_jpeg_decode_query_workspace", d, out.device, (low["workspace_bytes"],), (),
                             lambda got, want: "mm_jpeg_decode_query_workspace gives %d bytes, lower_jpeg_decode %d" % (got[0], want[0]))
    N.call("mm_jpeg_decode", out.device, d)
    return ws


def _decode_into(low, out, strict):
    """upload, launch, and the status (n) int32 on the device"""
    host, dev_buf, b0 = _upload(low, out.device)
    ws = _launch(low, host, dev_buf, b0, out)
    status = ws[low["status_offset"]:low["status_offset"] + 4 * low["n"]].view(torch.int32)
    if strict:
        bad = [(i, s) for i, s in enumerate(status.tolist()) if s]
        if bad:
            raise ValueError("damaged entropy-coded data in %d of %d files: %s" % (len(bad), low["n"], ", ".join("file %d: %s" % (i, status_text(s)) for i, s in bad[:16])
                                                                                  + (", ..." if len(bad) > 16 else "")))
    return status


def decode_jpeg(files, mode="RGB", device=None, out=None, strict=True):
    """Baseline JPEG files as device frames, Pillow's pixels: a ``DecodedFrames``.

    files    a list of ``bytes`` / ``bytearray`` / paths, or a ``JpegBatch`` (``encode_jpeg``'s result)
    mode     "RGB": what ``Image.open(f).convert('RGB')`` gives, (H,W,3); a greyscale file replicates its plane.  "L": greyscale files
             only, as ``.convert('L')`` of them, (H,W); a colour file is a ValueError.
    device   where to decode (default: ``out``'s device, else the current device)
    out      a dense uint8 device tensor of exactly the bytes needed (3 or 1 per pixel of all files), decoded in place; it may start at any
             byte.  Default: a fresh buffer.
    strict   True: wait for the status and raise ValueError listing the files whose entropy-coded data is damaged (the frames are decoded
             all the same, into ``out`` if given).  False: nothing waits; ``status`` says which files are damaged, and their pixels are
             ``decode_jpeg_host``'s.

    One upload (tables and bytes in one buffer), one memset and three launches, independent of the number of files; no per-file host
    work after parsing.  ValueError for what the parser rejects (see the module's docstring), naming the file's index: nothing is launched
    for a rejected batch."""
    low = files if isinstance(files, dict) else lower_jpeg_decode(files, mode)
    nbytes = int(low["offsets"][-1]) * low["channels"]
    if out is None:
        dev = torch.device("cuda" if device is None else device)
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != nbytes:
            raise ValueError("out must be a dense uint8 tensor of exactly %d bytes, got %s" % (nbytes, "%s %s" % (out.dtype, tuple(out.shape)) if torch.is_tensor(out) else type(out)))
        if device is not None and torch.device(device).type != out.device.type:
            raise ValueError("out is on %s, device says %s" % (out.device, device))
    N.require_device(out)
    flat = out.view(-1)
    status = _decode_into(low, flat, strict)
    return DecodedFrames(flat, low["offsets"], low["sizes"], status, low["mode"])
