"""The PNG file decoder on the MI355X (``decode_png`` over csrc/mm_png_decode.hip): whole tensors, torch.equal, no tolerance -- integers on
both sides.

Yardsticks: ``decode_png_host`` (which tests/test_png_decode_host.py holds to Pillow, to zlib and to the sanitized stand-alone build of the
kernel's inflate text) and live Pillow.  One mixed batch per output mode holds the whole clean host corpus -- mixed sizes, colour types,
depths, block types, every constructed stream -- plus 65 and 257 copies of a 13 x 3 file (more files than lanes, more than one dispatch's
worth of waves).  ``out=`` starts at every byte alignment between canaries, and so does the workspace's end.  The damaged vectors are
drawn from the host corpus, which has passed the restatement's range checks and the sanitized program, and they run last."""
import importlib
import io

import numpy as np
import pytest
import torch

import png_stream_cases as PSC
import stream_order as SO
from test_gpu_export import DEV, to_dev
from test_png_decode_host import MODES, clean_corpus, damaged_corpus, host, render_like, small_file

pytestmark = pytest.mark.gpu

PD = importlib.import_module("3d-magic-mirror_amd.png_decode")
PNG = importlib.import_module("3d-magic-mirror_amd.png")
J = importlib.import_module("3d-magic-mirror_amd.jpeg")
IB = importlib.import_module("3d-magic-mirror_amd.input_batches")

try:
    from PIL import Image
except ImportError:
    Image = None

_HOST = {}


def corpus(mode):
    """(names, files, decode_png_host's frames) of the clean corpus in ``mode``, made once"""
    if mode not in _HOST:
        pairs = clean_corpus(mode)
        frames, status = host(pairs, mode)
        assert not status.any()
        _HOST[mode] = ([n for n, _ in pairs], [f for _, f in pairs], frames)
    return _HOST[mode]


@pytest.mark.parametrize("mode", MODES)
def test_the_whole_clean_corpus_in_one_mixed_batch(mode):
    names, files, want = corpus(mode)
    files = files + [small_file()] * 65
    got = PD.decode_png(files, mode, device=DEV)
    assert got.status.cpu().tolist() == [0] * len(files) and got.images.dtype == torch.uint8 and got.images.dim() == 1
    assert got.images.numel() == PNG.MODES[mode][0] * got.offsets[-1] and len(set(map(tuple, got.sizes.tolist()))) > 10
    for name, f, w, g in zip(names, files, want, got.frames):
        assert torch.equal(g.cpu(), torch.from_numpy(w)), (mode, name)
        if Image is not None:
            assert torch.equal(g.cpu(), torch.from_numpy(np.array(Image.open(io.BytesIO(f)).convert(mode)))), (mode, name)
    copy = torch.from_numpy(host([small_file()], mode)[0][0])
    for g in got.frames[len(names):]:
        assert torch.equal(g.cpu(), copy)
    again = PD.decode_png(files, mode, device=DEV)                            # bit-identical on a second call
    assert torch.equal(again.images, got.images) and torch.equal(again.status, got.status)
    with pytest.raises(ValueError, match="different sizes"):
        got.stack()


def test_257_copies_span_the_dispatch():
    f = small_file()
    got = PD.decode_png([f] * 257, "L", device=DEV)
    want = torch.from_numpy(host([f])[0][0])
    assert got.stack().shape == (257, 13, 3) and torch.equal(got.stack().cpu(), want[None].expand(257, -1, -1)) and not got.status.any()


def test_out_and_workspace_between_canaries_at_every_byte_alignment():
    names, files, frames = corpus("RGB")
    pick = [k for k, n in enumerate(names) if n.startswith(("conv_", "filter_t2", "own_RGB_3x5", "three_types"))]
    files = [files[k] for k in pick]
    want = torch.cat([torch.from_numpy(frames[k]).reshape(-1) for k in pick])
    low = PD.lower_png_decode(files, "RGB")
    starts = 3 * low["offsets"][:-1]
    assert set(int(s) % 4 for s in starts) == {0, 1, 2, 3}
    wb = low["workspace_bytes"]
    for lead in range(4):
        storage = torch.full((want.numel() + 128 + 4,), 0xA5, dtype=torch.uint8, device=DEV)
        out = storage[64 + lead:64 + lead + want.numel()]
        assert out.data_ptr() % 4 == lead
        got = PD.decode_png(files, "RGB", device=DEV, out=out)
        assert got.images.data_ptr() == out.data_ptr() and torch.equal(out.cpu(), want), lead
        assert (storage[:64 + lead] == 0xA5).all() and (storage[64 + lead + want.numel():] == 0xA5).all()      # nothing outside out is written
        ws = torch.full((wb + 128,), 0xA5, dtype=torch.uint8, device=DEV)
        out.fill_(0)
        status = PD._decode_into(low, out, True, workspace=ws[64:64 + wb])
        assert not status.any() and torch.equal(out.cpu(), want)
        assert (ws[:64] == 0xA5).all() and (ws[64 + wb:] == 0xA5).all()                                         # nor outside workspace_bytes
    for bad in (torch.empty(want.numel() + 1, dtype=torch.uint8, device=DEV), torch.empty(want.numel(), dtype=torch.int8, device=DEV),
                torch.empty(2 * want.numel(), dtype=torch.uint8, device=DEV)[::2]):
        with pytest.raises(ValueError, match="out must be"):
            PD.decode_png(files, "RGB", device=DEV, out=bad)


@pytest.mark.parametrize("mode,shape", [("RGB", (3, 5)), ("RGB", (64, 65)), ("L", (3, 5)), ("L", (64, 65)), ("RGBA", (3, 5)), ("RGBA", (64, 65))])
def test_a_png_batch_straight_from_encode_png_decodes_to_its_frames(mode, shape):
    H, W = shape
    x = np.stack([render_like(H, W, seed=s) for s in range(3)])
    frames = x[..., 0] if mode == "L" else x if mode == "RGB" else np.concatenate([x, 255 - x[..., :1]], 3)
    dev = to_dev(torch.from_numpy(np.ascontiguousarray(frames)))
    batch = PNG.encode_png(dev, mode)
    got = PD.decode_png(batch, mode, device=DEV)
    assert torch.equal(got.stack(), dev) and not got.status.any()


def pool_inputs():
    rng = np.random.default_rng(9)
    shapes = ((17, 23), (16, 33), (8, 8), (31, 18))
    photos = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    jpegs = [J.encode_jpeg(to_dev(torch.from_numpy(p[None])), 90)[0] for p in photos]
    arrays = [f.cpu().numpy() for f in importlib.import_module("3d-magic-mirror_amd.jpeg_decode").decode_jpeg(jpegs, device=DEV).frames]
    return shapes, jpegs, arrays, rng


@pytest.mark.parametrize("mask", (None, "market", "alpha"))
def test_image_pool_from_files_then_assemble_batch(mask):
    import png_writer as PW
    shapes, jpegs, arrays, rng = pool_inputs()
    if mask == "alpha":
        rgba = [np.concatenate([rng.integers(0, 256, (h, w, 3), dtype=np.uint8), (rng.integers(0, 3, (h, w, 1)) * 100).astype(np.uint8)], 2) for h, w in shapes]
        pngs = [PW.png_of(a, 8, 6, (1, 4)) for a in rgba]
        segs = [((a[..., 3] > 0) * 255).astype(np.uint8) for a in rgba]
    else:
        grey = [(rng.integers(0, 3, (h, w)) * 90).astype(np.uint8) for h, w in shapes]
        pngs = [PW.png_of(a, 8, 0, (2, 3)) for a in grey[:2]] + [PW.png_of(a // 90, 2, 3, (0,), plte=bytes([0, 0, 0, 90, 90, 90, 180, 180, 180])) for a in grey[2:]]
        segs = [((a > 0) * 255).astype(np.uint8) for a in grey] if mask == "market" else grey
    ref = IB.ImagePool(arrays, segs, DEV)
    pool = IB.ImagePool.from_files(jpegs, pngs, DEV, mask=mask)
    assert torch.equal(pool.buffer, ref.buffer)
    assert np.array_equal(pool.sizes, ref.sizes) and np.array_equal(pool.offsets, ref.offsets)
    idx = [3, 0, 2, 1]
    aug = IB.draw_augmentation("cub", pool.sizes[idx], rng=__import__("random").Random(3))
    assert torch.equal(IB.assemble_batch(pool, idx, (32, 32), "cub", aug), IB.assemble_batch(ref, idx, (32, 32), "cub", aug))
    with pytest.raises(ValueError, match="image 1: the photo is"):
        IB.ImagePool.from_files(jpegs, [pngs[0], pngs[0]] + pngs[2:], DEV, mask=mask)
    with pytest.raises(ValueError, match="mask must be"):
        IB.ImagePool.from_files(jpegs, pngs, DEV, mask="bird")


def test_on_a_delayed_side_stream_the_bits_are_the_default_streams():
    c = SO.BY_NAME[PSC.NAME]
    SO.run_behind_delay(c.make_inputs, c.op, syncs=False, name=None)


def test_zz_damaged_files_return_status_and_the_host_decoders_pixels():
    """(last in the file: every vector is a stream the host restatement's range checks and the sanitized program have passed)"""
    by_name = {n: f for n, f, _ in damaged_corpus()}
    trunc = sorted((n for n in by_name if n.startswith("trunc_")), key=lambda n: int(n[6:]))
    names = ["bad_block_btype3", "bad_block_nlen", "bad_code_286", "bad_code_d30", "bad_code_unassigned", "bad_distance", "short", "short_stored",
             "overrun_stored", "cl_oversubscribed", "cl_incomplete", "ll_oversubscribed", "ll_incomplete", "dd_oversubscribed", "dd_incomplete",
             "no_end_of_block", "repeat_at_the_start", "repeat_past_the_end", "too_many_lengths", "bad_filter", "flip_3", "flip_100"]
    names += [trunc[k] for k in np.linspace(0, len(trunc) - 6, 8).astype(int)]
    files = [by_name[n] for n in names] + [small_file()]
    assert len(files) <= 64
    frames, status = PD.decode_png_host(files)
    seen = 0
    for s in status.tolist():
        seen |= s
    assert seen == 127 and status[-1] == 0 and (status != 0).sum() >= 28       # (a flipped bit may leave a valid stream: then only pixels differ)
    low = PD.lower_png_decode(files)
    nbytes, wb = int(low["offsets"][-1]), low["workspace_bytes"]
    storage = torch.full((nbytes + 128,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.full((wb + 128,), 0xA5, dtype=torch.uint8, device=DEV)
    out = storage[64:64 + nbytes]
    got_status = PD._decode_into(low, out, False, workspace=ws[64:64 + wb])
    assert got_status.cpu().tolist() == status.tolist()
    assert torch.equal(out.cpu(), torch.cat([torch.from_numpy(f).reshape(-1) for f in frames]))
    assert (storage[:64] == 0xA5).all() and (storage[64 + nbytes:] == 0xA5).all() and (ws[:64] == 0xA5).all() and (ws[64 + wb:] == 0xA5).all()
    with pytest.raises(ValueError) as e:
        PD.decode_png(files, "L", device=DEV)
    assert str(e.value) == "damaged data in %d of %d files: %s" % (int((status != 0).sum()), len(files), ", ".join("file %d: %s" % (i, PD.status_text(s)) for i, s in enumerate(status.tolist()) if s))
    got = PD.decode_png(files, "L", device=DEV, strict=False)
    assert [i for i, s in enumerate(got.status.cpu().tolist()) if s] == [i for i, s in enumerate(status.tolist()) if s]
