"""The PNG encoder on the MI355X (csrc/mm_png.hip) against the restatement (tests/test_png_host.py): every file of the device equals the
restatement's byte for byte -- nothing on either side is floating point and every atomic is an integer OR or XOR, so there is no
tolerance.  Where Pillow imports it also decodes the device's own files, back to the frames to the bit.

The cases are test_png_host's constructed ones (each reaches what it is named for: asserted there).  Beyond them: an ``export_grid`` sheet
of a tiny ``render_views`` call and the mask and RGBA frames of ``export_images`` go straight in; 256 x 256 x 4 uniform noise makes both
Adler sums wrap and gives the IDAT many CRC pieces in several workgroups; rows of 50..56 literals give IDATs (and type + data) of
PNG_CRC_PIECE - 1, PNG_CRC_PIECE and PNG_CRC_PIECE + 1 bytes; frames start at every byte alignment and come through other strides."""
import ctypes
import importlib
import io
import os

import numpy as np
import pytest
import torch

from conftest import TEMPLATES
from test_gpu_export import to_dev
from test_png_host import CASES, Image, S, as_frames, chunks_of, noise, png_restated, render_like

pytestmark = pytest.mark.gpu

P = importlib.import_module("3d-magic-mirror_amd.png")
EX = importlib.import_module("3d-magic-mirror_amd.export")


def differ(got, want):
    if len(got) != len(want):
        return "lengths %d and %d" % (len(got), len(want))
    at = next(i for i in range(len(got)) if got[i] != want[i])
    return "first difference at byte %d of %d: %02x, not %02x" % (at, len(got), got[at], want[at])


def held(frames, dev_frames=None, **kw):
    """encode_png of the frames (host uint8 array or tensor) gives the restatement's files; Pillow reads the device's back as the frames"""
    host = np.asarray(frames.cpu() if torch.is_tensor(frames) else frames)
    mode = kw.get("mode", "RGB")
    x = to_dev(torch.from_numpy(np.ascontiguousarray(host))) if dev_frames is None else dev_frames
    before = x.clone()
    batch = P.encode_png(x, **kw)
    want = png_restated(host, mode, kw.get("filter", "adaptive"), kw.get("segment"))
    f = as_frames(host, mode)
    assert isinstance(batch, P.PngBatch) and len(batch) == len(want) == f.shape[0]
    assert batch.shape == tuple(host.shape[:host.ndim - (2 if mode == "L" else 3)])
    assert batch.offsets[0] == 0 and batch.offsets[-1] == len(batch.buffer) == sum(len(w) for w in want)
    for i, w in enumerate(want):
        got = batch[i]
        assert got == w, "file %d: %s" % (i, differ(got, w))
        if Image is not None:
            im = Image.open(io.BytesIO(got))
            assert im.mode == mode and im.size == (f.shape[2], f.shape[1])
            assert np.array_equal(np.asarray(im), f[i][..., 0] if mode == "L" else f[i]), "file %d: Pillow reads other pixels" % i
    assert torch.equal(x, before), "the frames are left as they were"
    return batch


@pytest.mark.parametrize("name", list(CASES))
def test_constructed_cases(name):
    frames, kw = CASES[name]
    held(frames, **kw)


def test_single_frame_is_a_batch_of_one_and_writes(tmp_path):
    f = render_like(7, 5)
    x = to_dev(torch.from_numpy(f))
    b = P.encode_png(x)
    assert b.shape == () and len(b) == 1 and b[0] == P.encode_png(x[None])[0] == png_restated(f)[0]
    b.write([tmp_path / "one.png"])
    assert (tmp_path / "one.png").read_bytes() == b[0]


def test_the_same_call_twice_gives_the_same_bytes():
    x = to_dev(torch.from_numpy(np.stack([render_like(33, 47, s) for s in range(5)])))
    a, b = P.encode_png(x, segment=1024), P.encode_png(x, segment=1024)
    assert a.offsets == b.offsets and bytes(a.buffer.numpy()) == bytes(b.buffer.numpy())


def renders(pkg, size, B=2, n=3):
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), size)
    att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, B, size, size, seed=0)
    a = {k: att[k].to("cuda:0") for k in ("vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases")}
    a["azimuths"] = (a["azimuths"][:, None] + torch.arange(n, device="cuda:0", dtype=torch.float32)[None] * 120.0).contiguous()
    with torch.no_grad():
        frames, _ = dr.render_views(no_mask=False, **a)
    return frames


def test_export_grid_of_render_views_goes_straight_in(pkg):
    sheet = EX.export_grid(renders(pkg, 32), rounding="nearest")
    assert sheet.shape[0] == 3 and sheet.dtype == torch.uint8 and sheet.is_cuda
    held(sheet.cpu().numpy(), sheet)
    assert pkg.encode_png(sheet, filter=0, segment=1024)[2] == png_restated(sheet.cpu().numpy(), "RGB", 0, 1024)[2]


def test_mask_and_rgba_of_export_images_go_straight_in(pkg):
    x = renders(pkg, 64, B=1, n=2)
    mask = EX.export_images(x, "mask")
    rgba = EX.export_images(x, "rgba")
    assert mask.shape == (1, 2, 64, 64) and rgba.shape == (1, 2, 64, 64, 4)
    assert held(mask.cpu().numpy(), mask, mode="L").shape == (1, 2)
    assert held(rgba.cpu().numpy(), rgba, mode="RGBA").shape == (1, 2)


def test_noise_wraps_adler_and_fills_many_crc_pieces():
    f = noise((256, 256, 4), 12)
    b = held(f, mode="RGBA")
    idat = chunks_of(b[0])[1][1]
    assert len(idat) > 256 * P.PNG_CRC_PIECE * 4                          # several workgroups' worth of pieces
    assert f.astype(np.int64).sum() > 65521 and len(b[0]) <= P.lower_png(256, 256, "RGBA")["file_capacity"]


def test_idat_lengths_around_a_crc_piece():
    lengths = set()
    for W in range(P.PNG_CRC_PIECE - 14, P.PNG_CRC_PIECE - 7):             # 8-bit literals only: the IDAT holds W + 9 bytes, the CRC covers W + 13
        row = (1 + (np.arange(W) * 37) % 140).astype(np.uint8).reshape(1, 1, W)
        b = held(row, mode="L", filter=0)
        lengths.add(len(chunks_of(b[0])[1][1]))
    piece = P.PNG_CRC_PIECE
    assert {piece - 5, piece - 4, piece - 3, piece - 1, piece, piece + 1} <= lengths      # the first three: type + data is piece - 1, piece, piece + 1


def test_every_byte_alignment_and_strides():
    base = torch.from_numpy(np.stack([render_like(5, 7, s) for s in range(4)]))          # 105 bytes per frame
    flat = torch.zeros(4 * 105 + 8, dtype=torch.uint8, device="cuda:0")
    for shift in range(4):
        flat[shift:shift + 420] = to_dev(base).reshape(-1)
        held(base, flat[shift:shift + 420].view(4, 5, 7, 3))
    grey = torch.from_numpy(noise((3, 5, 7), 3))
    odd = torch.zeros(3 * 35 + 2, dtype=torch.uint8, device="cuda:0")
    odd[1:106] = to_dev(grey).reshape(-1)
    assert odd[1:].data_ptr() % 2 == 1
    held(grey, odd[1:106].view(3, 5, 7), mode="L")
    wide = to_dev(torch.from_numpy(np.stack([render_like(5, 14, s) for s in range(4)])))
    view = wide[:, :, ::2]                                                               # every other column: goes through .contiguous()
    assert not view.is_contiguous()
    held(view.cpu().numpy(), view)
    planes = to_dev(base).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)            # (n,H,W,3) over planar memory
    assert not planes.is_contiguous()
    held(base, planes)


def test_many_segments_in_flight_at_each_segment_length():
    frames = np.stack([np.roll(render_like(64, 96, 7), 3 * i, axis=1) for i in range(6)])
    for seg in (1024, 2048, 4096):
        held(frames, segment=seg)


def test_queries_are_lower_pngs(pkg):
    N = pkg._native
    d = N.MMPngDesc()
    for n, H, W, mode, seg in ((36, 64, 96, "RGB", S), (1, 1, 1, "L", 1), (48, 256, 128, "RGB", 1024), (2, 300, 200, "RGBA", P.PNG_MAX_SEGMENT)):
        low = P.lower_png(H, W, mode, seg)
        d.n, d.H, d.W, d.channels, d.filter, d.segment = n, H, W, low["channels"], -1, seg
        assert N.fn("mm_png_query_workspace")(ctypes.byref(d)) == low["workspace_bytes"](n)
        assert N.fn("mm_png_files_offset")(ctypes.byref(d)) == low["files_offset"](n)
