"""Renders blended into backgrounds by Poisson (seamless-cloning) editing, as 8-bit frames: host side of ``mm_poisson_frames``
(csrc/mm_poisson.hip).

The fourth way the reference pastes a render into a dataset frame: poisson_image_editing.py, which tool/generate_market_test.py:44
imports and never calls, because it solves one ``scipy.sparse.linalg.spsolve`` per frame and per channel on the host behind a ``.cpu()``.
Here the same system (poisson_image_editing.py:33-108 with offset (0,0)) is solved for all the frames of a batch in ONE launch, by a fixed
number of red-black SOR sweeps over a plane that never leaves the LDS of its workgroup, and comes back as one byte-sized copy.

Per frame: ``s`` the render's rgb, ``t`` the background behind the reflection pad resized back to (H,W) -- bit for bit
``pyramid_frames``' level-0 background, no blur --, ``in`` the mask.  Cells outside the mask are pinned to ``t``; with
``border="reference"`` those on the image's outer row or column are not (the reference's ``range(1, n - 1)`` loops leave them a Laplacian
row against their target value, so a corner comes out at about half its target), with ``border="pinned"`` every one is.  Every other
cell satisfies ``4 x_p - sum x_q = b_p`` over its 4-neighbours inside the image, with ``b_p = 4 s_p - sum s_q`` inside the mask and
``b_p = t_p`` outside.  The host lowers a call to the two resize tables (``lower_poisson``); DESIGN.md has the order of the solve in full.

The solution leaves [0, 1] (about -0.6 ... 1.5 on uniform inputs): the quantiser saturates and sends NaN to 0, as ``export_images`` does.

Out of scope: a non-zero source offset (the reference's ``warpAffine``); mixed gradients; quantising ``s`` and ``t`` to bytes before the
solve (the reference works on uint8 images, this call on the floats it is given; the system is linear in them); the reference's random
streams; gradients; planes that do not fit LDS (256 x 256 does not; a banded or multi-workgroup solve); JPEG encoding, which is
``encode_jpeg`` (jpeg.py).  Device tensors only."""
import functools
import math

import numpy as np
import torch

from . import _native as N
from .frames import LDS_BYTES, ROWS, _check_inputs, _launch, _lower_common, _rows, resize_taps

BORDERS = {"reference": 0, "pinned": 1}        # MMPoissonDesc.border

# the call site (the script imports the blend next to the pyramid's, with the same background path)
PRESETS = {"tool/generate_market_test": dict(bg_pad=16)}


def default_omega(H, W):
    """the SOR factor of the model problem on N = max(H, W): 2 / (1 + sin(pi / (N + 1))), formed in fp64 and rounded to fp32"""
    return float(np.float32(2.0 / (1.0 + math.sin(math.pi / (max(int(H), int(W)) + 1)))))


def default_sweeps(H, W):
    return max(4 * max(int(H), int(W)), 32)


def lds_bytes(low):
    """bytes of LDS the kernel takes for a lowered call (include/mm_render.h, MMPoissonDesc): mm::poisson_lds_bytes in Python.  Two
    compacted colour planes of (H + 2) rows of (W + 3) // 2 words, and W times the most source rows that the vertical resize of a band
    of 8 output rows reads, each rounded up to 4 floats."""
    H, W = low["H"], low["W"]
    _, _, t, b = low["bg_pad"]
    start, count = low["bg_y"][0].numpy(), low["bg_y"][1].numpy()
    rows = 0
    for y0 in range(0, H, ROWS):
        y1 = min(y0 + ROWS, H)
        lo, hi = int(start[y0:y1].min()), int((start[y0:y1] + count[y0:y1]).max())
        c_lo = min(max(lo, 0), H + t + b - 1)
        rows = max(rows, min(max(hi - 1, 0), H + t + b - 1) - c_lo + 1)
    plane = ((H + 2) * ((W + 3) // 2) + 3) // 4 * 4
    return 4 * (2 * plane + (rows * W + 3) // 4 * 4)


@functools.lru_cache(maxsize=32)
def _geometry(H, W, pad, antialias):
    """what a call's sizes alone decide, kept between calls: the two resize tables, their rows packed for the kernel, and the LDS the
    kernel takes.  The tensors are shared between the calls that hit the cache: read, not written."""
    l, r, t, b = pad
    geo = dict(bg_y=resize_taps(H + t + b, H, antialias), bg_x=resize_taps(W + l + r, W, antialias))
    geo["rows"] = np.concatenate([_rows(geo[key]).reshape(-1) for key in ("bg_y", "bg_x")])
    geo["lds_bytes"] = lds_bytes(dict(geo, H=H, W=W, bg_pad=pad))
    return geo


def lower_poisson(H, W, n_fg, n_bg, bg_index, fg_index=None, *, bg_pad=16, antialias=False, border="reference", sweeps=None, omega=None):
    """A call as the tables the kernel reads (host arithmetic only; nothing is launched and the arguments are left untouched): a dict of
    fg_index, bg_index (B,) int32; bg_y, bg_x, each ``resize_taps`` of the padded axis; the sizes; border; sweeps and omega with their
    defaults filled in (omega as the fp32 value the kernel gets); lds_bytes; and ``params``, all of it packed as MMPoissonDesc.params
    wants it (int32 words, floats by their bits).  Raises ValueError for what the kernel refuses: see ``poisson_frames``."""
    if border not in BORDERS:
        raise ValueError("border must be 'reference' or 'pinned', got %r" % (border,))
    low, fgi, bgi, _ = _lower_common(H, W, n_fg, n_bg, bg_index, fg_index, bg_pad, taps=lambda B: None)
    H, W, pad = low["H"], low["W"], low["bg_pad"]
    sweeps = default_sweeps(H, W) if sweeps is None else int(sweeps)
    if sweeps < 0 or sweeps > N.POISSON_MAX_SWEEPS:
        raise ValueError("sweeps must be in [0, %d], got %r" % (N.POISSON_MAX_SWEEPS, sweeps))
    omega = default_omega(H, W) if omega is None else float(np.float32(omega))
    if not 0.0 < omega < 2.0:
        raise ValueError("omega must lie inside (0, 2), got %r" % (omega,))
    geo = _geometry(H, W, pad, bool(antialias))
    if geo["lds_bytes"] > LDS_BYTES:
        raise ValueError("the call takes %d bytes of LDS, more than %d: the whole %d x %d plane stays in one workgroup's LDS for the "
                         "solve; a smaller image" % (geo["lds_bytes"], LDS_BYTES, H, W))
    low.update(antialias=bool(antialias), border=border, sweeps=sweeps, omega=omega, bg_y=geo["bg_y"], bg_x=geo["bg_x"], lds_bytes=geo["lds_bytes"])
    low["params"] = torch.from_numpy(np.concatenate([fgi, bgi, geo["rows"]]))
    return low


def _check_mask(mask, renders):
    want = tuple(renders.shape[:-3]) + tuple(renders.shape[-2:])
    if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError("mask must be a bool or uint8 tensor, got %s" % (mask.dtype if torch.is_tensor(mask) else type(mask),))
    if tuple(mask.shape) != want:
        raise ValueError("mask must have the renders' shape without the channels, %s, got %s" % (want, tuple(mask.shape)))


def poisson_frames(renders, backgrounds, bg_index, *, fg_index=None, mask=None, bg_pad=16, antialias=False, border="reference", sweeps=None,
                   omega=None, rounding="trunc", as_float=False):
    """Frames of the Poisson blend as 8-bit pixels, all in one launch: (...,H,W,3) uint8, the dimensions of ``bg_index`` in front.

        t = resize(reflection_pad(background));  s = render rgb;  inside = mask, or trunc(alpha * 255) != 0
        x = t on the pinned cells;  4 x_p - sum_q x_q = (4 s_p - sum_q s_q if inside else t_p) on the free ones, q inside the image

    renders, backgrounds, bg_index, fg_index, bg_pad, antialias, rounding, as_float
                 exactly as in ``composite_frames`` and ``pyramid_frames``: float (...,4,H,W) renders, dense NCHW or NHWC memory read in
                 place, leading dimensions kept; float (n_bg,3|4,H,W) backgrounds; the background (and, with fg_index, the render) of
                 each frame; the reflection pad as an int or (left, right, top, bottom), resized back to (H,W), no blur; as_float gives
                 the quantised values as (...,3,H,W) float32 ``q / 255``.
    mask         None: inside is ``trunc(alpha * 255) != 0`` on the render's channel 3, the byte ``export_images(rounding="trunc")``
                 stores followed by the reference's ``mask[mask != 0] = 1``.  Otherwise a bool or uint8 device tensor with the renders'
                 leading dimensions and (H,W), non-zero meaning inside; a frame takes the mask of its render (``fg_index``).
    border       "reference": the cells outside the mask on the image's outer row or column are free, with b = t, as the reference's
                 loops leave them (a corner outside the mask comes out at about half its target); "pinned": every cell outside the
                 mask is t -- the mode for clean frames.
    sweeps, omega  red-black SOR: x starts at t; per sweep the free cells with (y + x) even, then those with (y + x) odd, each
                 ``x += omega * ((b + ((l + r) + (u + d))) * 0.25 - x)`` in fp32.  Defaults, with N = max(H, W): omega
                 2 / (1 + sin(pi / (N + 1))), sweeps max(4 N, 32), which leave the fp32 iterate within 1e-5 of the fp64 direct solve
                 (tests/test_poisson_host.py).  The count is fixed: no convergence test, nothing synchronises or comes back.

    The whole plane stays in LDS for the solve: a call beyond 160 KiB (``lds_bytes``; 256 x 256 does not fit) raises ValueError and
    launches nothing.  ValueError also: mismatched shapes, a mask of another shape or type, an index outside its range, a reflection pad
    not smaller than the dimension it reflects in, an unknown border or rounding, sweeps < 0, omega outside (0, 2).  Not differentiable;
    the inputs are left unmodified; bitwise reproducible.

        frames = poisson_frames(pred, Xa, torch.randint(0, B, (B,)), **PRESETS["tool/generate_market_test"])
        for f in frames.cpu().numpy(): PIL.Image.fromarray(f).save(...)                 # ONE device-to-host copy"""
    _, H, W, n_fg, shape = _check_inputs(renders, backgrounds, bg_index, fg_index, rounding)
    if mask is not None:
        _check_mask(mask, renders)
    low = lower_poisson(H, W, n_fg, backgrounds.shape[0], bg_index, fg_index, bg_pad=bg_pad, antialias=antialias, border=border, sweeps=sweeps, omega=omega)
    d = N.MMPoissonDesc()
    d.border, d.sweeps, d.omega = BORDERS[border], low["sweeps"], low["omega"]
    if mask is not None:
        N.require_device(mask)
        mask = mask.detach().contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        d.mask = N.ptr(mask)
    return _launch(d, "mm_poisson_frames", low, renders, backgrounds, shape, H, W, rounding, as_float)
