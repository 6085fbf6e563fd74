"""Assembly of training batches from resident 8-bit images (3d-magic-mirror_amd/input_batches.py, csrc/mm_batch.hip) without a GPU:
the numpy restatement of the canonical record -- Pillow's antialiased bicubic in its 22-bit fixed point, two passes with the clamp to
bytes between them, Pillow's nearest, the threshold, to_tensor's divide and the composite -- that tests/test_gpu_input_batches.py
holds the kernel to bit for bit; the restatement against the recorded outputs of the reference's own loaders
(tests/golden/input_batches.npz) and against live Pillow; draw_augmentation against the recorded draws; the lowering of both
recipes; the C ABI's mirror and return codes; every ValueError."""
import ctypes
import importlib
import os
import random

import numpy as np
import pytest

IB = importlib.import_module("3d-magic-mirror_amd.input_batches")
N = importlib.import_module("3d-magic-mirror_amd._native")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "input_batches.npz")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def _cubic(t):
    a = -0.5
    if t < 0.0:
        t = -t
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def tap_table(n_in, n_out):
    """per output index: (first tap, the taps' 22-bit integer weights); double arithmetic as Pillow's precompute_coeffs orders it"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    inv = 1.0 / fs
    table = []
    for xx in range(n_out):
        c = (xx + 0.5) * scale
        xmin = max(0, int(c - support + 0.5))
        xmax = min(n_in, int(c + support + 0.5))
        w = [_cubic((x - c + 0.5) * inv) for x in range(xmin, xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        table.append((xmin, np.array([int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w], dtype=np.int64)))
    return table


def _pass(src, n_out):
    """one resampling pass along axis 0 of a uint8 array, to clamped bytes"""
    out = np.zeros((n_out,) + src.shape[1:], dtype=np.uint8)
    s = src.astype(np.int64)
    for xx, (xmin, k) in enumerate(tap_table(src.shape[0], n_out)):
        acc = (1 << 21) + np.tensordot(k, s[xmin:xmin + len(k)], axes=(0, 0))
        out[xx] = np.clip(acc >> 22, 0, 255)
    return out


def bicubic(canvas, Wr, Hr):
    """(Hc,Wc,3) uint8 -> (Hr,Wr,3) uint8: the horizontal pass to bytes, then the vertical pass on those bytes"""
    h = _pass(canvas.transpose(1, 0, 2), Wr).transpose(1, 0, 2)
    return _pass(h, Hr)


def nearest_table(n_in, n_out):
    """source index per output index, -1 where Pillow leaves the output pixel untouched: (int)xo, xo = a / 2 stepped by a = in / out"""
    a = n_in / n_out
    xo = a * 0.5
    t = np.full(n_out, -1, dtype=np.int64)
    for x in range(n_out):
        xin = -1 if xo < 0.0 else int(xo)
        if 0 <= xin < n_in:
            t[x] = xin
        xo += a
    return t


def canvas_of(img, seg, r):
    """the canvas of a record, rgb (Hc,Wc,3) and mask (Hc,Wc): the (mirrored) source where the window, the clip rectangle and the image meet, 0 elsewhere"""
    if r[IB.REC_FLIP_SRC]:
        img, seg = img[:, ::-1], seg[:, ::-1]
    Hs, Ws = seg.shape
    x0, y0, Wc, Hc = (int(r[i]) for i in (IB.REC_X0, IB.REC_Y0, IB.REC_WC, IB.REC_HC))
    rgb, m = np.zeros((Hc, Wc, 3), dtype=np.uint8), np.zeros((Hc, Wc), dtype=np.uint8)
    xa, xb = max(x0, 0, int(r[IB.REC_CX0])), min(x0 + Wc, Ws, int(r[IB.REC_CX1]))
    ya, yb = max(y0, 0, int(r[IB.REC_CY0])), min(y0 + Hc, Hs, int(r[IB.REC_CY1]))
    if xa < xb and ya < yb:
        rgb[ya - y0:yb - y0, xa - x0:xb - x0] = img[ya:yb, xa:xb]
        m[ya - y0:yb - y0, xa - x0:xb - x0] = seg[ya:yb, xa:xb]
    return rgb, m


def assemble_restated(images, segs, records, out_hw, bg=False):
    """what input_batches.assemble_records returns, (B,4,H,W) float32, from host arrays"""
    H, W = out_hw
    out = np.zeros((len(records), 4, H, W), dtype=np.float32)
    for b, r in enumerate(records):
        rgb, m = canvas_of(images[r[IB.REC_IMG]], segs[r[IB.REC_IMG]], r)
        Wr, Hr = int(r[IB.REC_WR]), int(r[IB.REC_HR])
        q = bicubic(rgb, Wr, Hr)
        tx, ty = nearest_table(m.shape[1], Wr), nearest_table(m.shape[0], Hr)
        mq = np.where((ty[:, None] >= 0) & (tx[None, :] >= 0), m[np.maximum(ty, 0)[:, None], np.maximum(tx, 0)[None, :]], 0)
        mq = np.where(mq > 160, 255, 0).astype(np.uint8)
        # the shift and the output flip: a (H,W) frame over the resized image, 0 outside
        fq, fm = np.zeros((H, W, 3), dtype=np.uint8), np.zeros((H, W), dtype=np.uint8)
        xs = np.arange(W)
        rx = (W - 1 - xs if r[IB.REC_FLIP_OUT] else xs) + int(r[IB.REC_DX])
        ry = np.arange(H) + int(r[IB.REC_DY])
        okx, oky = (rx >= 0) & (rx < Wr), (ry >= 0) & (ry < Hr)
        ok = oky[:, None] & okx[None, :]
        cy, cx = np.clip(ry, 0, Hr - 1)[:, None], np.clip(rx, 0, Wr - 1)[None, :]
        fq[ok], fm[ok] = q[cy, cx][ok], mq[cy, cx][ok]
        v = fq.astype(np.float32) / np.float32(255.0)
        mask = fm.astype(np.float32) / np.float32(255.0)
        if not bg:
            v = np.where(fm[..., None] > 0, v, np.float32(1.0))
        out[b, :3], out[b, 3] = v.transpose(2, 0, 1), mask
    return out


# ---- live Pillow: the loaders' steps, written from their description ---------------------------------------------------------------------
def pillow_sample(img, seg, out_hw, recipe, aug, bg):
    from PIL import Image, ImageOps
    H, W = out_hw
    im, sg = Image.fromarray(img, "RGB"), Image.fromarray(seg, "L")
    cut = lambda p: p > 160 and 255
    if recipe == "cub":
        if aug is not None:
            flip, _, _, left, upper, right, lower = (int(v) for v in aug)
            if flip:
                im, sg = im.transpose(Image.FLIP_LEFT_RIGHT), sg.transpose(Image.FLIP_LEFT_RIGHT)
            im, sg = ImageOps.expand(im, 10), ImageOps.expand(sg, 10)
            im, sg = im.crop((left, upper, right, lower)), sg.crop((left, upper, right, lower))
        w, h = im.size
        d = max(w, h)
        pad = ((d - w) // 2, (d - h) // 2, d - w - (d - w) // 2, d - h - (d - h) // 2)
        im, sg = ImageOps.expand(im, pad), ImageOps.expand(sg, pad)
        im, sg = im.resize((W, H)), sg.resize((W, H), Image.NEAREST).point(cut)
    else:
        if aug is not None:
            left, upper, flip = (int(v) for v in aug)
            im, sg = im.resize((W, H)), sg.resize((W, H), Image.NEAREST).point(cut)
            im, sg = ImageOps.expand(im, 10), ImageOps.expand(sg, 10)
            im, sg = im.crop((left, upper, left + W, upper + H)), sg.crop((left, upper, left + W, upper + H))
            if flip:
                im, sg = im.transpose(Image.FLIP_LEFT_RIGHT), sg.transpose(Image.FLIP_LEFT_RIGHT)
        im, sg = im.resize((W, H)), sg.resize((W, H), Image.NEAREST).point(cut)
    v = np.asarray(im, dtype=np.uint8).astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)
    m = np.asarray(sg, dtype=np.uint8).astype(np.float32)[None] / np.float32(255.0)
    rgb = v if bg else v * m + np.ones_like(v) * (1 - m)
    return np.concatenate([rgb, m], 0)


def noise_image(rng, Hs, Ws):
    """noise bytes with a quarter 0 and a quarter 255 (the clamp between the passes), a mask around the threshold"""
    img = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    u = rng.random((Hs, Ws, 3))
    img[u < 0.25], img[u > 0.75] = 0, 255
    seg = rng.choice(np.array([0, 159, 160, 161, 255], dtype=np.uint8), (Hs, Ws))
    return img, seg


@pytest.mark.parametrize("recipe", IB.RECIPES)
def test_restatement_equals_live_pillow(recipe):
    pytest.importorskip("PIL")
    rng, pr = np.random.default_rng(5), random.Random(5)
    bad = 0
    for case in range(300):
        Hs, Ws = (int(v) for v in rng.integers(5, 65, 2)) if case % 10 else (int(rng.integers(5, 401)), int(rng.integers(5, 401)))
        H = int(rng.choice([16, 32, 48, 128] if case % 10 == 0 else [16, 32]))
        out_hw = (H, H) if recipe == "cub" else (H, H // 2)
        img, seg = noise_image(rng, Hs, Ws)
        aug = IB.draw_augmentation(recipe, [(Hs, Ws)], pr) if case % 3 else None
        rec = IB.lower_batch([(Hs, Ws)], [0], out_hw, recipe, aug)
        got = assemble_restated([img], [seg], rec, out_hw, bg=bool(case & 1))[0]
        want = pillow_sample(img, seg, out_hw, recipe, None if aug is None else aug[0], bool(case & 1))
        bad += int((got != want).sum())
    assert bad == 0


# ---- the recorded loader outputs ---------------------------------------------------------------------------------------------------------
def golden_cases():
    g = np.load(GOLDEN)
    for k in range(int(g["n_cases"])):
        p = "c%02d_" % k
        yield {"recipe": str(g[p + "recipe"]), "train": bool(g[p + "train"]), "bg": bool(g[p + "bg"]), "seed": int(g[p + "seed"]),
               "out_hw": tuple(int(v) for v in g[p + "out_hw"]), "images": [g[p + "img%d" % i] for i in range(int(g[p + "n"]))],
               "segs": [g[p + "seg%d" % i] for i in range(int(g[p + "n"]))], "draws": g[p + "draws"], "out": g[p + "out"]}


def golden_records(c):
    sizes = [s.shape for s in c["segs"]]
    return IB.lower_batch(sizes, np.arange(len(sizes)), c["out_hw"], c["recipe"], c["draws"] if c["train"] else None)


def test_golden_covers_both_recipes_and_flags():
    seen = {(c["recipe"], c["train"], c["bg"]) for c in golden_cases()}
    assert seen == {(r, t, b) for r in IB.RECIPES for t in (False, True) for b in (False, True)}
    assert {c["out_hw"] for c in golden_cases()} == {(16, 16), (32, 32), (32, 16)}
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_restatement_reproduces_every_golden_tensor():
    for c in golden_cases():
        got = assemble_restated(c["images"], c["segs"], golden_records(c), c["out_hw"], c["bg"])
        assert got.dtype == c["out"].dtype and np.array_equal(got, c["out"]), (c["recipe"], c["train"], c["bg"])


def test_draw_augmentation_reproduces_the_recorded_draws():
    n = 0
    for c in golden_cases():
        if c["train"]:
            got = IB.draw_augmentation(c["recipe"], [s.shape for s in c["segs"]], random.Random(c["seed"]))
            assert got.dtype == np.int32 and np.array_equal(got, c["draws"]), c["recipe"]
            n += 1
    assert n >= 4
    random.seed(11)
    a = IB.draw_augmentation("cub", [(48, 64)] * 3)                       # the module's own generator is the default
    assert np.array_equal(a, IB.draw_augmentation("cub", [(48, 64)] * 3, random.Random(11)))


# ---- the restatement's own edges -----------------------------------------------------------------------------------------------------------
def test_same_size_pass_is_the_identity_and_taps_sum_to_one():
    for n_in, n_out in ((7, 7), (500, 128), (5, 32), (1, 16), (256, 16)):
        for xmin, k in tap_table(n_in, n_out):
            assert 0 <= xmin and xmin + len(k) <= n_in and len(k) >= 1
            assert abs(int(k.sum()) - (1 << 22)) <= len(k)
            assert len(k) <= IB._ksize(n_in, n_out)
    src = np.random.default_rng(0).integers(0, 256, (7, 4, 3), dtype=np.uint8)
    assert np.array_equal(_pass(src, 7), src)


def test_the_clamp_between_the_passes_is_visible():
    rng = np.random.default_rng(1)
    img, _ = noise_image(rng, 40, 40)
    two = bicubic(img, 16, 16)
    h = np.zeros((40, 16, 3))
    for xx, (xmin, k) in enumerate(tap_table(40, 16)):
        h[:, xx] = np.tensordot(k / float(1 << 22), img[:, xmin:xmin + len(k)].astype(np.float64), axes=(0, 1))
    one = np.zeros((16, 16, 3))
    for yy, (ymin, k) in enumerate(tap_table(40, 16)):
        one[yy] = np.tensordot(k / float(1 << 22), h[ymin:ymin + len(k)], axes=(0, 0))
    assert np.abs(np.clip(np.rint(one), 0, 255) - two).max() >= 2


def test_nearest_table():
    assert nearest_table(4, 8).tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    assert nearest_table(8, 4).tolist() == [1, 3, 5, 7]
    assert nearest_table(1, 3).tolist() == [0, 0, 0]
    for n_in, n_out in ((37, 16), (90, 32), (5, 32), (256, 16)):
        t = nearest_table(n_in, n_out)
        assert t.min() >= -1 and t.max() < n_in


# ---- lowering ---------------------------------------------------------------------------------------------------------------------------------
def test_cub_lowering_keeps_the_crop_as_the_clip_rectangle():
    # a 40 x 30 image (W x H); the crop cuts 4 columns on the left and 3 rows at the bottom, then the square padding brings back window
    # over pixels the crop removed: they must stay 0
    aug = np.array([[1, 0, 0, 14, 10, 60, 37]], dtype=np.int32)
    r = IB.lower_batch([(30, 40)], [0], (16, 16), "cub", aug)[0]
    assert r[IB.REC_FLIP_SRC] == 1 and r[IB.REC_FLIP_OUT] == 0 and (r[IB.REC_DX], r[IB.REC_DY]) == (0, 0)
    assert (r[IB.REC_CX0], r[IB.REC_CY0], r[IB.REC_CX1], r[IB.REC_CY1]) == (4, 0, 50, 27)
    assert (r[IB.REC_WC], r[IB.REC_HC]) == (46, 46) and (r[IB.REC_X0], r[IB.REC_Y0]) == (4, 0 - (46 - 27) // 2)
    assert (r[IB.REC_WR], r[IB.REC_HR]) == (16, 16)
    img = np.full((30, 40, 3), 200, dtype=np.uint8)
    seg = np.full((30, 40), 255, dtype=np.uint8)
    rgb, m = canvas_of(img, seg, r)
    assert rgb.shape == (46, 46, 3)
    y0 = (46 - 27) // 2
    assert (m[y0:y0 + 27, :36] == 255).all() and m[:y0].max() == 0 and m[y0 + 27:].max() == 0 and m[:, 36:].max() == 0
    # rows y0 + 27 .. y0 + 29 of the window lie over image rows 27 .. 29, which the crop removed
    assert y0 + 27 - y0 < 30 and rgb[y0 + 27:y0 + 30].max() == 0


def test_cub_lowering_without_augmentation_pads_the_image_to_a_square():
    rec = IB.lower_batch([(30, 41), (7, 5)], [0, 1], (32, 32), "cub")
    assert rec[0, [IB.REC_X0, IB.REC_Y0, IB.REC_WC, IB.REC_HC]].tolist() == [0, -5, 41, 41]
    assert rec[1, [IB.REC_X0, IB.REC_Y0, IB.REC_WC, IB.REC_HC]].tolist() == [-1, 0, 7, 7]
    assert rec[0, [IB.REC_CX0, IB.REC_CY0, IB.REC_CX1, IB.REC_CY1]].tolist() == [0, 0, 41, 30]
    assert rec[:, IB.REC_IMG].tolist() == [0, 1] and rec[:, IB.REC_FLIP_SRC].tolist() == [0, 0]


def test_market_lowering():
    aug = np.array([[0, 20, 1], [10, 10, 0]], dtype=np.int32)
    rec = IB.lower_batch([(128, 64)], [0, 0], (32, 16), "market", aug)
    assert rec[0, [IB.REC_X0, IB.REC_Y0, IB.REC_WC, IB.REC_HC, IB.REC_WR, IB.REC_HR]].tolist() == [0, 0, 64, 128, 16, 32]
    assert rec[0, [IB.REC_DX, IB.REC_DY, IB.REC_FLIP_OUT, IB.REC_FLIP_SRC]].tolist() == [-10, 10, 1, 0]
    assert rec[1, [IB.REC_DX, IB.REC_DY, IB.REC_FLIP_OUT]].tolist() == [0, 0, 0]
    plain = IB.lower_batch([(128, 64)], [0], (32, 16), "market")
    assert plain[0, [IB.REC_DX, IB.REC_DY, IB.REC_FLIP_OUT]].tolist() == [0, 0, 0]
    assert plain[0, [IB.REC_CX0, IB.REC_CY0, IB.REC_CX1, IB.REC_CY1]].tolist() == [0, 0, 64, 128]


def test_pool_packs_without_padding():
    rng = np.random.default_rng(2)
    pairs = [noise_image(rng, h, w) for h, w in ((1, 1), (5, 7), (37, 23))]
    pool = IB.ImagePool([p[0] for p in pairs], [p[1] for p in pairs])
    assert len(pool) == 3 and pool.offsets.dtype == np.int64 and pool.offsets.tolist() == [0, 1, 36, 36 + 37 * 23]
    assert pool.sizes.dtype == np.int32 and pool.sizes.tolist() == [[1, 1], [5, 7], [37, 23]]
    assert pool.images.numel() == 3 * pool.offsets[-1] and pool.segs.numel() == pool.offsets[-1]
    assert np.array_equal(pool.images.numpy()[3:3 + 105], pairs[1][0].reshape(-1))
    assert np.array_equal(pool.segs.numpy()[36:], pairs[2][1].reshape(-1))
    assert pool.offsets_dev.tolist() == pool.offsets.tolist() and pool.sizes_dev.tolist() == pool.sizes.tolist()
    assert pool.images.data_ptr() == pool.buffer.data_ptr()                    # views of the one buffer


# ---- ValueErrors ------------------------------------------------------------------------------------------------------------------------------
def _pool():
    rng = np.random.default_rng(3)
    pairs = [noise_image(rng, 12, 9), noise_image(rng, 6, 20)]
    return IB.ImagePool([p[0] for p in pairs], [p[1] for p in pairs])


def test_value_errors():
    pool = _pool()
    with pytest.raises(ValueError, match="idx"):
        IB.assemble_batch(pool, [0, 2], (16, 16), "cub")
    with pytest.raises(ValueError, match="idx"):
        IB.assemble_batch(pool, [-1], (16, 16), "cub")
    with pytest.raises(ValueError, match="idx"):
        IB.assemble_batch(pool, [], (16, 16), "cub")
    with pytest.raises(ValueError, match="recipe"):
        IB.assemble_batch(pool, [0], (16, 16), "birds")
    with pytest.raises(ValueError, match="recipe"):
        IB.draw_augmentation("birds", pool.sizes)
    with pytest.raises(ValueError, match="aug"):
        IB.assemble_batch(pool, [0, 1], (16, 16), "cub", aug=np.zeros((2, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="aug"):
        IB.assemble_batch(pool, [0, 1], (32, 16), "market", aug=np.zeros((1, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="aug"):
        IB.assemble_batch(pool, [0], (16, 16), "cub", aug=np.zeros((1, 7), dtype=np.float32))
    with pytest.raises(ValueError, match="empty"):
        IB.assemble_batch(pool, [0], (16, 16), "cub", aug=np.array([[0, 0, 0, 12, 3, 12, 20]], dtype=np.int32))
    with pytest.raises(ValueError, match="out_hw"):
        IB.assemble_batch(pool, [0], (0, 16), "cub")
    with pytest.raises(ValueError, match="ratio cap"):
        IB.assemble_batch(pool, [1], (1, 1), "cub")                           # 20 -> 1
    with pytest.raises(ValueError, match="uint8"):
        IB.ImagePool([np.zeros((4, 4, 3), dtype=np.float32)], [np.zeros((4, 4), dtype=np.uint8)])
    with pytest.raises(ValueError, match="uint8"):
        IB.ImagePool([np.zeros((4, 4, 3), dtype=np.uint8)], [np.zeros((4, 5), dtype=np.uint8)])
    with pytest.raises(ValueError, match="same length"):
        IB.ImagePool([], [])


def _record(**kw):
    r = np.zeros((1, IB.REC_INTS), dtype=np.int32)
    r[0, [IB.REC_WC, IB.REC_HC, IB.REC_CX1, IB.REC_CY1, IB.REC_WR, IB.REC_HR]] = (9, 12, 9, 12, 16, 16)
    for k, v in kw.items():
        r[0, getattr(IB, "REC_" + k)] = v
    return r


def test_record_checks():
    IB.check_records(_record(), 2, (16, 16))
    IB.check_records(_record(WC=256, HC=256), 2, (16, 16))                    # exactly at the cap
    for bad, what in ((_record(WC=257), "ratio cap"), (_record(HC=257), "ratio cap"), (_record(IMG=2), "image indices"),
                      (_record(WC=0), "empty"), (_record(HR=0), "empty"), (_record(FLIP_SRC=2), "flags"), (_record(FLIP_OUT=-1), "flags"),
                      (_record(X0=1 << 25), "2\\^24"), (_record().astype(np.int64), "int32"), (_record()[:, :15], "int32")):
        with pytest.raises(ValueError, match=what):
            IB.check_records(bad, 2, (16, 16))
    with pytest.raises(ValueError, match="LDS"):
        IB.check_records(_record(WC=4096, HC=4096, WR=256, HR=256), 2, (256, 256))
    assert IB.lds_bytes(_record(WC=1024, HC=1024, WR=128, HR=128), (128, 128)) < 64 * 1024
    assert IB.lds_bytes(_record(WC=16 * 190, HC=16 * 190, WR=190, HR=190), (190, 190)) <= IB.LDS_BYTES


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------
def _desc(rec, keep):
    d = N.MMBatchDesc()
    d.B, d.H, d.W, d.n_images, d.bg = rec.shape[0], 16, 16, 2, 0
    rec = np.ascontiguousarray(rec)
    keep.append(rec)
    fake = ctypes.c_void_p(256)                                               # never dereferenced: every refusal comes before any GPU work
    d.images = d.segs = d.offsets = d.sizes = d.records = d.out = fake
    d.records_host = ctypes.c_void_p(rec.ctypes.data)
    return d


def test_abi_mirror_and_return_codes():
    L = N.lib()
    assert L.mm_abi_version() == 9
    assert L.mm_struct_size(30) == ctypes.sizeof(N.MMBatchDesc) and L.mm_struct_size(31) == 0
    assert "mm_assemble_batch" in N.EXPORTS
    keep = []
    call = lambda d: L.mm_assemble_batch(ctypes.byref(d), None)
    assert L.mm_assemble_batch(None, None) == -1
    for field in ("images", "segs", "offsets", "sizes", "records", "records_host", "out"):
        d = _desc(_record(), keep)
        setattr(d, field, None)
        assert call(d) == -1, field
    for field in ("B", "H", "W", "n_images"):
        d = _desc(_record(), keep)
        setattr(d, field, 0)
        assert call(d) == -2, field
    for bad in (_record(IMG=2), _record(IMG=-1), _record(WC=0), _record(HC=-3), _record(WR=0), _record(HR=0), _record(FLIP_SRC=2),
                _record(FLIP_OUT=-1), _record(X0=(1 << 24) + 1), _record(DY=-(1 << 24) - 1)):
        assert call(_desc(bad, keep)) == -2
    assert call(_desc(_record(WC=257), keep)) == -5
    assert call(_desc(_record(HC=257), keep)) == -5
    d = _desc(_record(WC=4096, HC=4096, WR=256, HR=256), keep)
    d.H = d.W = 256
    assert call(d) == -5                                                      # within the ratio cap, beyond the LDS
    two = np.concatenate([_record(), _record(HC=257)])
    assert call(_desc(two, keep)) == -5                                       # every record is looked at
