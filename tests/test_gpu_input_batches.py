"""Batch assembly on the MI355X (csrc/mm_batch.hip) against the numpy restatement (tests/test_input_batches_host.py, itself held to live
Pillow and to the recorded loader outputs) and against those recorded outputs, with torch.equal: the resize is integer arithmetic on
tap weights formed by + - * / in fp64, the last step one correctly rounded fp32 divide, and the file is compiled without contraction,
so there is no tolerance to measure.

Shapes are the smallest that reach each path.  The pool's sources are 1x1, 5x7, 37x23 and 61x90 (H x W): 3 * W * H is odd for the
first three, so images start at every byte alignment.  The row tile is 8: output heights 16 and 32 are whole tiles, 8 exactly one, 13
ends in a partial tile; every case with more than one tile makes neighbouring workgroups recompute the overlap.  The ratios go from a
16-fold upscale (1 -> 16) to the cap of 16:1 (a 256 wide window -> 16) on each axis on its own."""
import importlib

import numpy as np
import pytest
import torch

from test_input_batches_host import assemble_restated, golden_cases, golden_records, noise_image

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
IB = importlib.import_module("3d-magic-mirror_amd.input_batches")
SHAPES = ((1, 1), (5, 7), (37, 23), (61, 90))
_STATE = {}


def sources():
    """the pool and its host arrays, made once; the mask of image 2 holds only the threshold's neighbours 160 and 161"""
    if not _STATE:
        rng = np.random.default_rng(7)
        pairs = [noise_image(rng, h, w) for h, w in SHAPES]
        pairs[2] = (pairs[2][0], rng.choice(np.array([160, 161], dtype=np.uint8), SHAPES[2]))
        _STATE["imgs"], _STATE["segs"] = [p[0] for p in pairs], [p[1] for p in pairs]
        _STATE["pool"] = IB.ImagePool(_STATE["imgs"], _STATE["segs"], DEV)
    return _STATE["pool"], _STATE["imgs"], _STATE["segs"]


def record(img, window, out_wh, clip=None, flip_src=0, dx=0, dy=0, flip_out=0):
    r = np.zeros(IB.REC_INTS, dtype=np.int32)
    Hs, Ws = SHAPES[img]
    r[IB.REC_IMG], r[IB.REC_FLIP_SRC], r[IB.REC_FLIP_OUT], r[IB.REC_DX], r[IB.REC_DY] = img, flip_src, flip_out, dx, dy
    r[IB.REC_X0:IB.REC_HC + 1] = window
    r[IB.REC_CX0:IB.REC_CY1 + 1] = clip if clip is not None else (0, 0, Ws, Hs)
    r[IB.REC_WR], r[IB.REC_HR] = out_wh
    return r


def check(records, out_hw, bg=False):
    pool, imgs, segs = sources()
    records = np.stack(records)
    got = IB.assemble_records(pool, records, out_hw, bg)
    assert got.shape == (len(records), 4) + tuple(out_hw) and got.dtype == torch.float32 and got.is_contiguous() and got.device == DEV
    want = torch.from_numpy(assemble_restated(imgs, segs, records, out_hw, bg))
    assert torch.equal(got.cpu(), want)
    return want


@pytest.mark.parametrize("bg", (False, True))
def test_golden_loader_outputs(bg):
    n = 0
    for c in golden_cases():
        if c["bg"] != bg:
            continue
        pool = IB.ImagePool(c["images"], c["segs"], DEV)
        got = IB.assemble_batch(pool, np.arange(len(pool)), c["out_hw"], c["recipe"], c["draws"] if c["train"] else None, bg)
        assert torch.equal(got.cpu(), torch.from_numpy(c["out"])), (c["recipe"], c["train"])
        assert torch.equal(IB.assemble_records(pool, golden_records(c), c["out_hw"], bg), got)
        n += 1
    assert n == 4


@pytest.mark.parametrize("out_hw", ((16, 16), (32, 16), (13, 16), (8, 24)))
@pytest.mark.parametrize("recipe", IB.RECIPES)
def test_recipes_on_every_source(recipe, out_hw):
    """every source size (each start alignment, up- and downscales of both axes at once) under both recipes, with and without draws;
    B = 5 with a repeated index"""
    import random
    pool, imgs, segs = sources()
    idx = np.array([0, 1, 2, 3, 1])
    for k, aug in enumerate((None, IB.draw_augmentation(recipe, pool.sizes[idx], random.Random(3)))):
        rec = IB.lower_batch(pool.sizes, idx, out_hw, recipe, aug)
        for bg in (False, True):
            got = IB.assemble_batch(pool, idx, out_hw, recipe, aug, bg)
            assert torch.equal(got.cpu(), torch.from_numpy(assemble_restated(imgs, segs, rec, out_hw, bg))), (k, bg)
            if aug is None:
                assert torch.equal(got[1], got[4])                        # the repeated index


def test_each_axis_scales_on_its_own():
    # 61x90 source: x down / y up, x up / y down, x same / y down, both down by non-integers; 5x7: both up
    recs = [record(3, (0, 0, 90, 10), (16, 16)), record(3, (0, 0, 10, 61), (16, 16)), record(3, (3, 0, 16, 61), (16, 16)),
            record(3, (0, 0, 90, 61), (16, 16)), record(1, (0, 0, 7, 5), (16, 16))]
    check(recs, (16, 16))
    check([record(3, (0, 0, 90, 61), (16, 32)), record(2, (0, 0, 23, 37), (16, 32))], (32, 16), bg=True)


def test_single_sample_single_pixel_source():
    want = check([record(0, (0, 0, 1, 1), (16, 16))], (16, 16), bg=True)      # B = 1, a 16-fold upscale of one pixel
    assert len(np.unique(want[0, 0].numpy())) == 1


def test_windows_over_every_edge_and_outside():
    w = (16, 16)
    recs = [record(2, (-9, 4, 20, 20), w), record(2, (12, 4, 20, 20), w), record(2, (2, -11, 20, 20), w), record(2, (2, 25, 20, 20), w),
            record(2, (-6, -6, 40, 50), w),                                   # over all four at once
            record(2, (23, 0, 10, 10), w), record(2, (-10, 0, 10, 10), w), record(2, (0, 37, 10, 10), w), record(2, (0, -10, 10, 10), w),
            record(2, (2, 2, 12, 12), w, clip=(30, 0, 40, 10)),               # inside the image, outside the clip rectangle
            record(2, (0, 0, 23, 37), w, clip=(5, 8, 17, 30)),                # the clip rectangle cuts image content inside the window
            record(2, (0, 0, 23, 37), w, clip=(9, 9, 9, 20))]                 # an empty clip rectangle
    want = check(recs, (16, 16), bg=True)
    for b in (5, 6, 7, 8, 9, 11):
        assert float(want[b].abs().max()) == 0.0                              # entirely outside: zeros (bg keeps them; over white they are 1)
    want = check(recs, (16, 16), bg=False)
    assert float(want[5, :3].min()) == 1.0 and float(want[5, 3].max()) == 0.0


def test_flips_and_shifts():
    w = (16, 24)
    recs = [record(3, (-4, 3, 70, 50), w, flip_src=fs, flip_out=fo, dx=dx, dy=dy)
            for fs in (0, 1) for fo in (0, 1) for dx, dy in ((0, 0), (10, -10), (-10, 10), (0, 10), (-10, 0))]
    check(recs, (24, 16))
    check([record(1, (0, 0, 7, 5), w, flip_src=1, flip_out=1, dx=3, dy=-2), record(1, (0, 0, 7, 5), w, dx=16, dy=0),
           record(1, (0, 0, 7, 5), w, dx=0, dy=-24)], (24, 16))               # the last two are shifted out of the resized image entirely


def test_threshold_neighbours():
    want = check([record(2, (0, 0, 23, 37), (23, 37))], (37, 23), bg=True)    # same size: the mask is the source's, thresholded
    _, _, segs = sources()
    assert np.array_equal(want[0, 3].numpy(), (segs[2] == 161).astype(np.float32))
    assert 0.25 < float(want[0, 3].mean()) < 0.75


def test_at_the_ratio_cap_and_beyond():
    pool, _, _ = sources()
    at = [record(3, (-80, -90, 256, 256), (16, 16)), record(3, (0, 0, 256, 16), (16, 16)), record(3, (0, 0, 16, 256), (16, 16))]
    check(at, (16, 16))
    for beyond in (record(3, (0, 0, 257, 16), (16, 16)), record(3, (0, 0, 16, 257), (16, 16))):
        with pytest.raises(ValueError, match="ratio cap"):
            IB.assemble_records(pool, np.stack([at[0], beyond]), (16, 16))
    d = IB.N.MMBatchDesc()                                                    # and the library itself refuses, before it launches
    rec = np.ascontiguousarray(np.stack([at[0], record(3, (0, 0, 257, 16), (16, 16))]))
    dev = torch.from_numpy(rec).to(DEV)
    out = torch.full((2, 4, 16, 16), 7.0, device=DEV)
    d.B, d.H, d.W, d.n_images = 2, 16, 16, len(pool)
    d.images, d.segs, d.offsets, d.sizes = IB.N.ptr(pool.images), IB.N.ptr(pool.segs), IB.N.ptr(pool.offsets_dev), IB.N.ptr(pool.sizes_dev)
    d.records_host, d.records, d.out = rec.ctypes.data, IB.N.ptr(dev), IB.N.ptr(out)
    import ctypes
    assert IB.N.lib().mm_assemble_batch(ctypes.byref(d), IB.N.current_stream(DEV)) == -5
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0


def test_wide_tables_beyond_64_kib_of_lds():
    rec = [record(3, (-100, -50, 1500, 1500), (128, 128))]                    # 11.7:1 to 128 x 128: 71 KiB of tables and rows
    assert 64 * 1024 < IB.lds_bytes(np.stack(rec), (128, 128)) <= IB.LDS_BYTES
    check(rec, (128, 128))


def test_other_stream_and_value_errors_on_the_device():
    pool, imgs, segs = sources()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        got = IB.assemble_batch(pool, [3, 2], (32, 16), "market", np.array([[0, 20, 1], [20, 0, 0]], dtype=np.int32))
    s.synchronize()
    rec = IB.lower_batch(pool.sizes, [3, 2], (32, 16), "market", np.array([[0, 20, 1], [20, 0, 0]], dtype=np.int32))
    assert torch.equal(got.cpu(), torch.from_numpy(assemble_restated(imgs, segs, rec, (32, 16))))
    with pytest.raises(ValueError, match="idx"):
        IB.assemble_batch(pool, [4], (16, 16), "cub")
    with pytest.raises(ValueError, match="recipe"):
        IB.assemble_batch(pool, [0], (16, 16), "atr")
