"""The GIF encoder on the MI355X (csrc/mm_gif.hip) against the restatement (tests/test_gif_host.py): the device's file equals the restatement's
byte for byte, whole file, and ``quantize_frames`` its palette and indices with torch.equal -- nothing on either side is floating point and
every atomic is an integer one, so there is no tolerance.  Where Pillow imports it also decodes the device's own file.

The cases are test_gif_host's constructed ones (each reaches what it is named for: asserted there).  Beyond them: 5 x 7 frames of 105 bytes
start at every byte alignment and come through non-contiguous strides; an ``export_grid`` result of a tiny ``render_views`` call goes
straight in; 36 frames of 64 x 96 keep several hundred segments and frames in flight; a 160 x 128 frame holds more white pixels (and more
of a second colour) than one workgroup of the histogram walks (256 lanes x 64 pixels), so runs are summed inside waves, across waves and
across workgroups; 300 x 300 noise fills nearly every bin, the median cut's largest table."""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import TEMPLATES
from test_gif_host import CASES, COLOURS, Image, S, gif_restated, noise, pillow_reads, quantize_restated, render_like
from test_gpu_export import to_dev

pytestmark = pytest.mark.gpu

G = importlib.import_module("3d-magic-mirror_amd.gif")
EX = importlib.import_module("3d-magic-mirror_amd.export")


def differ(got, want):
    if len(got) != len(want):
        return "lengths %d and %d" % (len(got), len(want))
    at = next(i for i in range(len(got)) if got[i] != want[i])
    return "first difference at byte %d of %d: %02x, not %02x" % (at, len(got), got[at], want[at])


def held(frames, dev_frames=None, **kw):
    """quantize_frames and encode_gif of the frames (host uint8 array or tensor) are the restatement's; Pillow reads the device's file"""
    host = np.asarray(frames.cpu() if torch.is_tensor(frames) else frames)
    host = host.reshape((-1,) + host.shape[-3:])
    x = to_dev(torch.from_numpy(np.ascontiguousarray(host))) if dev_frames is None else dev_frames
    before = x.clone()
    pal, idx = quantize_restated(host)
    got_pal, got_idx = G.quantize_frames(x)
    assert got_pal.shape == (256, 3) and got_idx.shape == host.shape[:3] and got_pal.dtype == got_idx.dtype == torch.uint8
    assert torch.equal(got_pal.cpu(), torch.from_numpy(pal)), "palette"
    assert torch.equal(got_idx.cpu(), torch.from_numpy(idx)), "indices"
    g = G.encode_gif(x, **kw)
    want = gif_restated(host, kw.get("delay", 10), kw.get("loop", 0), kw.get("segment", S), quantized=(pal, idx))
    got = bytes(g)
    assert got == want, differ(got, want)
    assert len(g) == len(want) and np.array_equal(g.palette, pal)
    assert torch.equal(x, before), "the frames are left as they were"
    if Image is not None:
        why = pillow_reads(got, pal, idx, kw.get("delay", 10), kw.get("loop", 0))
        assert why is None, why
    return g


@pytest.mark.parametrize("name", list(CASES))
def test_constructed_cases(name):
    frames, kw = CASES[name]
    held(frames, **kw)


def test_single_frame_is_a_batch_of_one(tmp_path):
    f = render_like(7, 5)
    x = to_dev(torch.from_numpy(f))
    g = G.encode_gif(x)
    assert bytes(g) == bytes(G.encode_gif(x[None])) == gif_restated(f)
    g.write(tmp_path / "one.gif")
    assert (tmp_path / "one.gif").read_bytes() == bytes(g)


def test_every_byte_alignment_and_strides():
    base = torch.from_numpy(np.stack([render_like(5, 7, s) for s in range(4)]))          # 105 bytes per frame
    flat = torch.zeros(4 * 105 + 8, dtype=torch.uint8, device="cuda:0")
    for shift in range(4):
        flat[shift:shift + 420] = to_dev(base).reshape(-1)
        held(base, flat[shift:shift + 420].view(4, 5, 7, 3))
    wide = to_dev(torch.from_numpy(np.stack([render_like(5, 14, s) for s in range(4)])))
    view = wide[:, :, ::2]                                                               # every other column: goes through .contiguous()
    assert not view.is_contiguous()
    held(view.cpu().numpy(), view)
    planes = to_dev(base).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)            # (n,H,W,3) over planar memory
    assert not planes.is_contiguous()
    held(base, planes)


def test_export_grid_of_render_views_goes_straight_in(pkg):
    B, n, size = 2, 3, 32
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), size)
    att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, B, size, size, seed=0)
    a = {k: att[k].to("cuda:0") for k in ("vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases")}
    a["azimuths"] = (a["azimuths"][:, None] + torch.arange(n, device="cuda:0", dtype=torch.float32)[None] * 120.0).contiguous()
    with torch.no_grad():
        frames, _ = dr.render_views(no_mask=False, **a)
    sheet = EX.export_grid(frames)
    assert sheet.shape[0] == n and sheet.dtype == torch.uint8 and sheet.is_cuda
    held(sheet.cpu().numpy(), sheet)
    assert bytes(pkg.encode_gif(sheet, delay=5, loop=None)) == gif_restated(sheet.cpu().numpy(), 5, None)


def test_many_segments_and_frames_in_flight():
    frames = np.stack([np.roll(render_like(64, 96, 7), 3 * i, axis=1) for i in range(36)])
    held(frames)
    held(frames, segment=512, delay=list(range(36)))


def test_more_pixels_in_a_bin_than_a_workgroup_walks():
    f = np.full((160, 128, 3), 255, dtype=np.uint8)                      # 20480 pixels, 16384 to a workgroup
    f[40:140, 30:33] = (250, 0, 7)                                       # runs that end inside a lane's walk
    f[60:62] = (17, 130, 201)
    f[100, 5::9] = COLOURS[(np.arange(len(f[100, 5::9])) * 11) % 256]
    held(f)
    two = np.zeros((1, 200, 256, 3), dtype=np.uint8)                     # two colours in two bins, half the frame each: equal counts
    two[:, 100:] = (8, 8, 8)
    g = held(two)
    assert np.array_equal(g.palette[:2], [[0, 0, 0], [8, 8, 8]]) and not g.palette[2:].any()


def test_noise_fills_the_median_cuts_table():
    f = noise(300 * 300 * 3, 11).astype(np.uint8).reshape(1, 300, 300, 3)
    pal, idx = quantize_restated(f)
    assert len(np.unique(idx)) == 256
    x = to_dev(torch.from_numpy(f))
    got_pal, got_idx = G.quantize_frames(x)
    assert torch.equal(got_pal.cpu(), torch.from_numpy(pal)) and torch.equal(got_idx.cpu(), torch.from_numpy(idx))
