"""Training batches assembled on the device from resident 8-bit images: host side of ``mm_assemble_batch`` (csrc/mm_batch.hip).

What the reference's DataLoader workers do per sample in Pillow (datasets/bird.py:69-136, datasets/market.py:77-145, atr.py like bird.py)
-- random flip, ``ImageOps.expand(10)``, random crop, pad to square, bicubic ``resize``, nearest ``resize`` of the mask, threshold at
160, ``to_tensor``, composite over white -- as ONE launch per batch, from decoded images that stay in device memory as bytes.  It is
the mirror of ``export.py``: bytes in, floats out.  The result is the loader's tensor bit for bit (integer arithmetic and one correctly
rounded fp32 divide; tests/test_input_batches_host.py holds the arithmetic to live Pillow and to recorded loader outputs).

    pool = ImagePool(images, segs, device)                       # once: lists of uint8 (H_i,W_i,3) and (H_i,W_i) arrays, one upload
    aug = draw_augmentation("cub", pool.sizes[idx], rng=random)  # host: the loader's own draws, in the loader's order
    Xa = assemble_batch(pool, idx, (128, 128), "cub", aug)       # (B,4,H,W) float32 on the device

``segs`` are what the reference's ``seg_loader`` returns (market's maps every non-zero byte to 255 when it loads; bird's thresholds at
160, which the threshold after the resize repeats).

The canonical per-sample record (16 int32; the kernel knows nothing else; ``lower_batch`` makes it from a recipe):

    REC_IMG                      source image
    REC_FLIP_SRC                 the source is read mirrored in x; every coordinate below is in the mirrored image
    REC_X0, REC_Y0, REC_WC, REC_HC   the canvas window, which may hang over any edge of the image
    REC_CX0, REC_CY0, REC_CX1, REC_CY1   the clip rectangle [cx0,cx1) x [cy0,cy1): a canvas pixel outside it or outside the image is 0
    REC_WR, REC_HR               the canvas is resized to (Wr,Hr): rgb by Pillow's antialiased bicubic, mask by Pillow's nearest, > 160
    REC_DX, REC_DY               output pixel (x,y) reads resized (x + dx, y + dy), 0 outside
    REC_FLIP_OUT                 ... of the output mirrored in x: (W - 1 - x + dx, y + dy)

then v = fl(q / 255), rgb = v where the mask is set and 1.0 elsewhere (unless ``bg``), channel 3 the mask as 0.0 / 1.0.

Limits (ValueError, nothing is launched): a resize ratio canvas / resized above RATIO_CAP = 16 on either axis (any upscale is allowed);
and the workgroup's tables and row buffer must fit the 160 KiB of LDS (``lds_bytes``): 1024 -> 128 at 8:1 takes 53 KiB, at the cap of
16:1 outputs at least 190 wide fit.  Nothing here is differentiable."""
import ctypes
import math
import random as _random

import numpy as np
import torch

from . import _native as N

RATIO_CAP = 16            # MM_BATCH_MAX_RATIO
ROW_TILE = 8              # MM_BATCH_ROWS: output rows per workgroup
LDS_BYTES = 160 * 1024
RECIPES = ("cub", "market")
(REC_IMG, REC_FLIP_SRC, REC_X0, REC_Y0, REC_WC, REC_HC, REC_CX0, REC_CY0, REC_CX1, REC_CY1, REC_WR, REC_HR, REC_DX, REC_DY,
 REC_FLIP_OUT) = range(15)
REC_INTS = 16
AUG_COLUMNS = {"cub": 7, "market": 3}     # cub: flip, w, h, left, upper, right, lower; market: left, upper, flip -- the order they are drawn in


class ImagePool:
    """Decoded images and masks resident on ``device`` as bytes.  All images are packed into one byte buffer and all masks into
    another, image i at pixel offset ``offsets[i]`` (byte 3 * offsets[i] of ``images``, byte offsets[i] of ``segs``): no per-image
    padding, so images start at any byte alignment.  ``offsets`` (N+1) int64 and ``sizes`` (N,2) int32 rows (H, W) are numpy arrays on
    the host; ``images``, ``segs``, ``offsets_dev`` and ``sizes_dev`` are views of ONE uploaded buffer.  ``device=None`` keeps the
    pool on the host (lowering and tests need no device)."""

    def __init__(self, images, segs, device=None):
        images, segs = list(images), list(segs)
        if not images or len(images) != len(segs):
            raise ValueError("images and segs must be two non-empty lists of the same length, got %d and %d" % (len(images), len(segs)))
        for i, (im, sg) in enumerate(zip(images, segs)):
            im, sg = np.asarray(im), np.asarray(sg)
            if im.dtype != np.uint8 or sg.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or sg.shape != im.shape[:2] or min(im.shape) < 1:
                raise ValueError("image %d: need uint8 arrays (H,W,3) and (H,W), got %s %s and %s %s" % (i, im.dtype, im.shape, sg.dtype, sg.shape))
            images[i], segs[i] = im, sg
        n = len(images)
        self.sizes = np.array([im.shape[:2] for im in images], dtype=np.int32).reshape(n, 2)
        self.offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(self.sizes[:, 0].astype(np.int64) * self.sizes[:, 1], out=self.offsets[1:])
        P = int(self.offsets[-1])
        tables = (4 * P + 7) // 8 * 8                          # the int64 table starts on an 8-byte boundary
        host = np.zeros(tables + 8 * (n + 1) + 8 * n, dtype=np.uint8)
        host[:3 * P] = np.concatenate([im.reshape(-1) for im in images])
        host[3 * P:4 * P] = np.concatenate([sg.reshape(-1) for sg in segs])
        host[tables:tables + 8 * (n + 1)] = self.offsets.view(np.uint8)
        host[tables + 8 * (n + 1):] = self.sizes.reshape(-1).view(np.uint8)
        self.device = None if device is None else torch.device(device)
        buf = torch.from_numpy(host)
        self.buffer = buf if self.device is None else buf.to(self.device)      # the one upload
        self.images, self.segs = self.buffer[:3 * P], self.buffer[3 * P:4 * P]
        self.offsets_dev = self.buffer[tables:tables + 8 * (n + 1)].view(torch.int64)
        self.sizes_dev = self.buffer[tables + 8 * (n + 1):].view(torch.int32).view(n, 2)

    @classmethod
    def from_jpeg(cls, files, segs, device):
        """The pool of JPEG ``files`` (a list of bytes / paths, or a ``JpegBatch``) decoded on ``device`` by ``decode_jpeg`` straight into
        the image region of the pool's one buffer: what ``ImagePool([np.asarray(Image.open(f).convert('RGB')) for f in files], segs, device)``
        holds, without the host decode and the 3 bytes a pixel of upload.  The masks and the two tables go up in one copy, the files' bytes in the
        decoder's, both from pinned memory on the current stream without waiting.  ValueError: what ``decode_jpeg`` rejects, masks that do not
        match the files' sizes, damaged files -- the one host wait of the call, ``decode_jpeg``'s strict wait for the status."""
        from . import jpeg_decode as JD
        if device is None:
            raise ValueError("ImagePool.from_jpeg decodes on a device; on the host, ImagePool(decode_jpeg_host(files)[0], segs)")
        low = JD.lower_jpeg_decode(files, "RGB")
        segs = [np.asarray(sg) for sg in segs]
        n = low["n"]
        if len(segs) != n:
            raise ValueError("files and segs must be two non-empty lists of the same length, got %d and %d" % (n, len(segs)))
        for i, sg in enumerate(segs):
            if sg.dtype != np.uint8 or sg.shape != tuple(low["sizes"][i]):
                raise ValueError("image %d: need a uint8 mask %s, got %s %s" % (i, tuple(low["sizes"][i]), sg.dtype, sg.shape))
        self = cls.__new__(cls)
        self.sizes, self.offsets, self.device = low["sizes"], low["offsets"], torch.device(device)
        P = int(self.offsets[-1])
        tables = (4 * P + 7) // 8 * 8                          # the layout of __init__'s buffer
        self.buffer = torch.empty(tables + 8 * (n + 1) + 8 * n, dtype=torch.uint8, device=self.device)
        head = np.zeros(self.buffer.numel() - 3 * P, dtype=np.uint8)          # everything behind the images: masks, padding, offsets, sizes
        head[:P] = np.concatenate([sg.reshape(-1) for sg in segs])
        head[tables - 3 * P:tables - 3 * P + 8 * (n + 1)] = self.offsets.view(np.uint8)
        head[tables - 3 * P + 8 * (n + 1):] = self.sizes.reshape(-1).view(np.uint8)
        self.images, self.segs = self.buffer[:3 * P], self.buffer[3 * P:4 * P]
        self.offsets_dev = self.buffer[tables:tables + 8 * (n + 1)].view(torch.int64)
        self.sizes_dev = self.buffer[tables + 8 * (n + 1):].view(torch.int32).view(n, 2)
        N.require_device(self.buffer)
        self.buffer[3 * P:].copy_(torch.from_numpy(head).pin_memory(), non_blocking=True)      # the masks and the tables: one upload, not waited for
        JD.decode_jpeg(low, out=self.images)                                # the files: the decoder's one upload, then straight into the image region
        return self

    @classmethod
    def from_files(cls, jpeg_files, png_masks, device, mask=None):
        """The pool of a dataset directory's two files per sample: the photos, JPEG ``jpeg_files``, through ``decode_jpeg`` and the masks, PNG
        ``png_masks``, through ``decode_png``, both straight into the pool's one buffer (each a list of bytes / paths, or a ``JpegBatch`` /
        ``PngBatch``).  Beside the files' bytes only the two small tables are uploaded.  mask: None keeps what ``Image.open(m).convert('L')``
        gives (bird.py, atr.py: the threshold after the resize follows); "market" maps every byte that is not 0 to 255 on the device
        (market.py's ``point(lambda p: p > 0 and 255)``); "alpha" decodes as ``.convert('RGBA')`` and keeps the alpha plane, not 0 as 255
        (thuman2.py).  What ``ImagePool(images, segs, device)`` holds for the same arrays, byte for byte.  ValueError: what the two decoders
        reject, masks whose sizes do not match the photos', damaged files (the decoders' strict waits for the status)."""
        from . import jpeg_decode as JD
        from . import png_decode as PD
        if device is None:
            raise ValueError("ImagePool.from_files decodes on a device")
        if mask not in (None, "market", "alpha"):
            raise ValueError("mask must be None, 'market' or 'alpha', got %r" % (mask,))
        low = JD.lower_jpeg_decode(jpeg_files, "RGB")
        lowm = PD.lower_png_decode(png_masks, "RGBA" if mask == "alpha" else "L")
        n = low["n"]
        if lowm["n"] != n:
            raise ValueError("jpeg_files and png_masks must be two non-empty lists of the same length, got %d and %d" % (n, lowm["n"]))
        for i in range(n):
            if tuple(lowm["sizes"][i]) != tuple(low["sizes"][i]):
                raise ValueError("image %d: the photo is %d x %d, its mask %d x %d" % ((i,) + tuple(low["sizes"][i]) + tuple(lowm["sizes"][i])))
        self = cls.__new__(cls)
        self.sizes, self.offsets, self.device = low["sizes"], low["offsets"], torch.device(device)
        P = int(self.offsets[-1])
        tables = (4 * P + 7) // 8 * 8                          # the layout of __init__'s buffer
        self.buffer = torch.zeros(tables + 8 * (n + 1) + 8 * n, dtype=torch.uint8, device=self.device)
        self.images, self.segs = self.buffer[:3 * P], self.buffer[3 * P:4 * P]
        self.offsets_dev = self.buffer[tables:tables + 8 * (n + 1)].view(torch.int64)
        self.sizes_dev = self.buffer[tables + 8 * (n + 1):].view(torch.int32).view(n, 2)
        N.require_device(self.buffer)
        tail = np.concatenate([self.offsets.view(np.uint8), self.sizes.reshape(-1).view(np.uint8)])
        self.buffer[tables:].copy_(torch.from_numpy(tail).pin_memory(), non_blocking=True)      # the two tables: one upload, not waited for
        JD.decode_jpeg(low, out=self.images)
        post = {None: 0, "market": N.PNG_POST_THRESHOLD, "alpha": N.PNG_POST_THRESHOLD | N.PNG_POST_ALPHA}[mask]
        PD._decode_into(lowm, self.segs, True, post=post)
        return self

    def __len__(self):
        return self.sizes.shape[0]


def draw_augmentation(recipe, sizes, rng=_random):
    """The loader's random draws for samples of ``sizes`` (B,2) rows (H, W), consumed from ``rng`` (a ``random.Random`` or the
    ``random`` module) with the calls and in the order of the reference's ``__getitem__``, sample after sample: (B,7) int32 rows
    (flip, w, h, left, upper, right, lower) for "cub", (B,3) rows (left, upper, flip) for "market"."""
    if recipe not in RECIPES:
        raise ValueError("recipe must be one of %s, got %r" % (", ".join(RECIPES), recipe))
    sizes = np.asarray(sizes).reshape(-1, 2)
    out = np.zeros((sizes.shape[0], AUG_COLUMNS[recipe]), dtype=np.int32)
    for b, (Hs, Ws) in enumerate(sizes.tolist()):
        if recipe == "cub":
            flip = rng.uniform(0, 1) < 0.5
            W, H = Ws + 20, Hs + 20
            w = rng.randint(int(0.95 * W), int(0.99 * W))
            h = rng.randint(int(0.95 * H), int(0.99 * H))
            left = rng.randint(0, W - w)
            upper = rng.randint(0, H - h)
            right = rng.randint(w - left, W)
            lower = rng.randint(h - upper, H)
            out[b] = (flip, w, h, left, upper, right, lower)
        else:
            left = rng.randint(0, 20)
            upper = rng.randint(0, 20)
            out[b] = (left, upper, rng.uniform(0, 1) < 0.5)
    return out


def lower_batch(sizes, idx, out_hw, recipe, aug=None):
    """The canonical records (B,16) int32 of a batch: ``sizes`` the pool's (N,2) table, ``idx`` the B sample indices (repeats allowed),
    ``aug`` the draws of ``draw_augmentation`` or None for the loader's train=False / aug=False path."""
    if recipe not in RECIPES:
        raise ValueError("recipe must be one of %s, got %r" % (", ".join(RECIPES), recipe))
    H, W = (int(v) for v in out_hw)
    if H < 1 or W < 1:
        raise ValueError("out_hw must be positive, got %r" % (out_hw,))
    sizes = np.asarray(sizes).reshape(-1, 2)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    if idx.size < 1 or idx.min() < 0 or idx.max() >= sizes.shape[0]:
        raise ValueError("idx must hold at least one index, all in [0, %d)" % sizes.shape[0])
    B = idx.size
    if aug is not None:
        aug = np.asarray(aug)
        if aug.shape != (B, AUG_COLUMNS[recipe]) or aug.dtype.kind not in "iub":
            raise ValueError("aug must be an integer (%d,%d) array for recipe %r, got %s %s" % (B, AUG_COLUMNS[recipe], recipe, aug.dtype, aug.shape))
        aug = aug.astype(np.int64)
    Hs, Ws = sizes[idx, 0].astype(np.int64), sizes[idx, 1].astype(np.int64)
    rec = np.zeros((B, REC_INTS), dtype=np.int64)
    rec[:, REC_IMG], rec[:, REC_WR], rec[:, REC_HR] = idx, W, H
    if recipe == "cub":
        if aug is None:
            cw, ch, cx, cy = Ws, Hs, 0, 0
        else:
            left, upper, right, lower = aug[:, 3], aug[:, 4], aug[:, 5], aug[:, 6]
            empty = (right <= left) | (lower <= upper)
            if empty.any():
                b = int(np.argmax(empty))
                raise ValueError("sample %d: the crop (%d,%d,%d,%d) is empty" % (b, left[b], upper[b], right[b], lower[b]))
            rec[:, REC_FLIP_SRC] = aug[:, 0] != 0
            cw, ch, cx, cy = right - left, lower - upper, left - 10, upper - 10
        d = np.maximum(cw, ch)
        rec[:, REC_X0], rec[:, REC_Y0], rec[:, REC_WC], rec[:, REC_HC] = cx - (d - cw) // 2, cy - (d - ch) // 2, d, d
        rec[:, REC_CX0], rec[:, REC_CY0], rec[:, REC_CX1], rec[:, REC_CY1] = cx, cy, cx + cw, cy + ch
    else:
        rec[:, REC_WC], rec[:, REC_HC], rec[:, REC_CX1], rec[:, REC_CY1] = Ws, Hs, Ws, Hs
        if aug is not None:
            rec[:, REC_DX], rec[:, REC_DY], rec[:, REC_FLIP_OUT] = aug[:, 0] - 10, aug[:, 1] - 10, aug[:, 2] != 0
    if np.abs(rec).max() > 1 << 24:
        raise ValueError("the draws put a coordinate beyond +-2^24")
    return rec.astype(np.int32)


def _ksize(n_in, n_out):
    return int(math.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1


def _ksizes(n_in, n_out):
    return np.ceil(2.0 * np.maximum(n_in / n_out, 1.0)).astype(np.int64) * 2 + 1


def lds_bytes(records, out_hw):
    """LDS of one workgroup for these records, as csrc/mm_batch.hip carves it: the two tap tables, the bounds and nearest tables and the
    row buffer of the horizontal pass, each sized by the largest sample of the batch."""
    rec = np.asarray(records).reshape(-1, REC_INTS).astype(np.float64)
    ksy = _ksizes(rec[:, REC_HC], rec[:, REC_HR])
    ksx = int(_ksizes(rec[:, REC_WC], rec[:, REC_WR]).max())
    rows = int((((ROW_TILE - 1) * (rec[:, REC_HC] / rec[:, REC_HR])).astype(np.int64) + ksy + 1).max())
    ksy, wr = int(ksy.max()), int(rec[:, REC_WR].max())
    return 4 * (wr * ksx + ROW_TILE * ksy + 3 * wr + 3 * ROW_TILE) + (rows * wr * 3 + 3) // 4 * 4


def check_records(records, n_images, out_hw):
    """ValueError for a record the kernel would refuse: an image out of range, an empty window or resize, a flag that is not 0 / 1, a
    resize ratio above RATIO_CAP or tables beyond the LDS."""
    rec = np.asarray(records)
    if rec.ndim != 2 or rec.shape[1] != REC_INTS or rec.shape[0] < 1 or rec.dtype != np.int32:
        raise ValueError("records must be an int32 (B,%d) array, got %s %s" % (REC_INTS, rec.dtype, rec.shape))
    H, W = (int(v) for v in out_hw)
    if H < 1 or W < 1:
        raise ValueError("out_hw must be positive, got %r" % (out_hw,))
    if rec[:, REC_IMG].min() < 0 or rec[:, REC_IMG].max() >= n_images:
        raise ValueError("record image indices must lie in [0, %d)" % n_images)
    if rec[:, [REC_WC, REC_HC, REC_WR, REC_HR]].min() < 1:
        raise ValueError("a record has an empty window or an empty resize")
    if rec[:, [REC_FLIP_SRC, REC_FLIP_OUT]].min() < 0 or rec[:, [REC_FLIP_SRC, REC_FLIP_OUT]].max() > 1:
        raise ValueError("record flags must be 0 or 1")
    if np.abs(rec[:, [REC_X0, REC_Y0, REC_CX0, REC_CY0, REC_CX1, REC_CY1, REC_DX, REC_DY]].astype(np.int64)).max() > 1 << 24 or rec[:, [REC_WC, REC_HC, REC_WR, REC_HR]].max() > 1 << 24:
        raise ValueError("record coordinates must lie within +-2^24")
    over = (rec[:, REC_WC] > RATIO_CAP * rec[:, REC_WR].astype(np.int64)) | (rec[:, REC_HC] > RATIO_CAP * rec[:, REC_HR].astype(np.int64))
    if over.any():
        b = int(np.argmax(over))
        r = rec[b]
        raise ValueError("sample %d: resizing %dx%d to %dx%d is beyond the ratio cap of %d:1" % (b, r[REC_WC], r[REC_HC], r[REC_WR], r[REC_HR], RATIO_CAP))
    if lds_bytes(rec, out_hw) > LDS_BYTES:
        raise ValueError("the tap tables and row buffer of this batch need %d bytes of LDS, more than %d" % (lds_bytes(rec, out_hw), LDS_BYTES))


def assemble_records(pool, records, out_hw, bg=False):
    """One launch: the (B,4,H,W) float32 batch of the canonical ``records`` (B,16) int32 (host array), dense NCHW on the pool's device.
    The table goes up as one non-blocking copy from pinned memory; nothing comes back and nothing waits."""
    records = np.ascontiguousarray(records)
    check_records(records, len(pool), out_hw)
    if pool.device is None:
        raise RuntimeError("this ImagePool was built without a device")
    N.require_device(pool.buffer)
    H, W = (int(v) for v in out_hw)
    B = records.shape[0]
    host, dev = N.upload_int32(records, pool.device)
    out = torch.empty((B, 4, H, W), dtype=torch.float32, device=pool.device)
    d = N.MMBatchDesc()
    d.B, d.H, d.W, d.n_images, d.bg = B, H, W, len(pool), int(bool(bg))
    d.images, d.segs, d.offsets, d.sizes = N.ptr(pool.images), N.ptr(pool.segs), N.ptr(pool.offsets_dev), N.ptr(pool.sizes_dev)
    d.records_host, d.records = ctypes.c_void_p(host.data_ptr()), N.ptr(dev)
    d.out = N.ptr(out)
    st = N.fn("mm_assemble_batch")(d, N.current_stream(pool.device))          # (not N.call: a refusal is a ValueError here)
    if st in (-2, -5):
        raise ValueError("mm_assemble_batch refused the records: %s (MMStatus %d)" % (N.fn("mm_status_string")(st).decode(), st))
    N.check(st, "mm_assemble_batch")
    return out


def assemble_batch(pool, idx, out_hw=(128, 128), recipe="cub", aug=None, bg=False):
    """The loader's batch for samples ``idx`` of ``pool``: (B,4,H,W) float32, rgb over white (``bg``: rgb as it is) and the mask, what
    ``torch.stack([dataset[i]['data']['images'] for i in idx])`` gives with the same draws.  ``aug`` from ``draw_augmentation``, or
    None for the train=False / aug=False path.  "cub" follows bird.py / atr.py and pads to a square before the resize to (W,H);
    "market" resizes the whole image to (W,H) = (image_size, 2 * image_size) and shifts by the crop."""
    return assemble_records(pool, lower_batch(pool.sizes, idx, out_hw, recipe, aug), out_hw, bg)
