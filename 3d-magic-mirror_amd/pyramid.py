"""Renders blended into backgrounds through a three-level Laplacian pyramid, as 8-bit frames: host side of ``mm_pyramid_frames``
(csrc/mm_pyramid.hip).

What the reference's tool/generate_market_test.py:326-369 does on the host, one image at a time, after every render -- per batch
``Resize(ReflectionPad2d(16)(Xa[:, :3]))``; per image nine ``GaussianBlur(kernel_size=7)`` calls that each draw their own sigma, three
cascaded on the mask, three on a random background, three on the render, four differences, the six-term blend
``bg3*(1-mask3) + obj3*mask3 + lbg2*(1-mask2) + lobj2*mask2 + lbg1*(1-mask1) + lobj1*mask1`` and ``np.uint8(x * 255)`` behind a
blocking ``.cpu()`` -- as ONE launch for all the frames of a batch, and one byte-sized copy to the host.

The host lowers a call to small tables (``lower_pyramid``) with frames.py's ``gaussian_taps`` and ``resize_taps``; no transcendental
runs on the device.  The device then runs, per frame and in fp32 with every operation rounded as written and every sum in ascending tap
order from 0: the reflection pad (index arithmetic) and separable resize (x, then y) of the background -- no blur before it, this call
site's order --; for each of the seven planes (mask, three background, three render) a cascade of three separable blurs (x, then y), each
reflecting at the (H,W) image's own edge and each rounded as written, so every level is made in full; the blend as Python evaluates the
reference's line, left to right; ``export_images``' quantiser.  DESIGN.md has the order in full.

The pyramid's sums leave [0, 1] (uniform inputs range over about -0.25 ... 1.25), where the reference's ``np.uint8`` of the value is
undefined: this kernel saturates to 0 / 255 and sends NaN to 0, as ``export_images`` does.

poisson_image_editing.py (imported by that script, never called) is ``poisson_frames`` (poisson.py).  Out of scope: the texture mix with the
mean-texture bank (:339);
reproducing the reference's random streams (the caller draws ``bg_index`` and the sigmas: ``draw_sigmas``); gradients; other
numbers of levels.  JPEG encoding: ``encode_jpeg`` (jpeg.py).  Device tensors only."""
import functools

import numpy as np
import torch

from . import _native as N
from .frames import LDS_BYTES, MAX_TAPS, ROW_WORDS, ROWS, _check_inputs, _launch, _lower_common, _rows, band_bytes_lds, draw_sigmas, gaussian_taps, resize_taps

LEVELS = 3              # MM_PYRAMID_LEVELS
MAX_KERNEL = 15         # MM_PYRAMID_MAX_KERNEL
KINDS = ("mask", "background", "render")      # the plane kinds, in the order the reference draws their sigmas
assert (ROWS, MAX_TAPS, ROW_WORDS) == (8, 8, 10)   # MM_PYRAMID_ROWS, MM_PYRAMID_MAX_TAPS, MM_PYRAMID_ROW_WORDS: the band and resize rows of frames.py

# the call site; a sigma of None is drawn per frame, plane kind and level (draw_sigmas), as GaussianBlur(7) without sigma draws it per call
PRESETS = {"tool/generate_market_test": dict(blur=(7, None), bg_pad=16)}


def preset(name, n, generator=None):
    """The keyword arguments of ``pyramid_frames`` for the reference's call site (``PRESETS``) and n frames: nine sigmas drawn per frame,
    in the reference's order -- mask 1-3, background 1-3, render 1-3 --, as an (n,3,3) array [frame][plane kind][level]."""
    kw = dict(PRESETS[name])
    k, sigma = kw["blur"]
    kw["blur"] = (k, draw_sigmas(9 * n, generator=generator).view(n, 3, 3) if sigma is None else sigma)
    return kw


def _taps(blur, n):
    """(n,3,3,k) float32 taps of a blur argument: (kernel_size, sigma) with sigma a float or (n,3,3), or ready taps (k,) / (3,3,k) / (n,3,3,k)"""
    if isinstance(blur, tuple) and len(blur) == 2 and not torch.is_tensor(blur[0]) and np.ndim(blur[0]) == 0:
        k = int(blur[0])
        if k < 1 or k > MAX_KERNEL or k % 2 == 0:
            raise ValueError("kernel_size must be odd and in [1, %d], got %r" % (MAX_KERNEL, blur[0]))
        sig = torch.as_tensor(blur[1], dtype=torch.float32).detach().cpu()
        if sig.dim() != 0 and tuple(sig.shape) != (n, 3, 3):
            raise ValueError("sigma must be a float or of shape (%d,3,3), [frame][plane kind][level], got %s" % (n, tuple(sig.shape)))
        t = gaussian_taps(k, sig.reshape(-1)).reshape(tuple(sig.shape) + (k,))
    else:
        t = torch.as_tensor(blur, dtype=torch.float32).detach().cpu()
    given = tuple(t.shape)
    if t.dim() in (1, 3):
        t = t.reshape((1,) * (4 - t.dim()) + given)
    if t.dim() != 4 or tuple(t.shape[:3]) not in ((1, 1, 1), (1, 3, 3), (n, 3, 3)) or t.shape[3] < 1 or t.shape[3] > MAX_KERNEL or t.shape[3] % 2 == 0:
        raise ValueError("blur must be (kernel_size, sigma) or taps of shape (k,), (3,3,k) or (%d,3,3,k) with k odd and at most %d, got %s"
                         % (n, MAX_KERNEL, given))
    return t.expand(n, 3, 3, -1).contiguous()


def _level_rows(y0, y1, r, H):
    """mm::pyramid_rows: the rows [lo, hi) of level 0 that the band [y0, y1) needs"""
    lo, hi = y0, y1
    for _ in range(LEVELS):
        lo, hi = max(lo - r, 0), min(hi + r, H)
    return lo, hi


def lds_bytes(low):
    """bytes of LDS the kernel takes for a lowered call (include/mm_render.h, MMPyramidDesc): mm::pyramid_lds_bytes in Python"""
    H, W = low["H"], low["W"]
    _, _, t, b = low["bg_pad"]
    start, count = low["bg_y"][0].numpy(), low["bg_y"][1].numpy()
    r, rows = low["taps"].shape[-1] // 2, 0
    for y0 in range(0, H, ROWS):
        lo, hi = _level_rows(y0, min(y0 + ROWS, H), r, H)
        a, e = int(start[lo:hi].min()), int((start[lo:hi] + count[lo:hi]).max())
        c_lo = min(max(a, 0), H + t + b - 1)
        rows = max(rows, hi - lo, min(max(e - 1, 0), H + t + b - 1) - c_lo + 1)
    cap = (rows * W + 3) // 4 * 4
    return 4 * (2 * cap + 10 * ((ROWS * W + 3) // 4 * 4)) + band_bytes_lds(W)


@functools.lru_cache(maxsize=32)
def _geometry(H, W, pad, k, antialias):
    """what a call's sizes alone decide, kept between calls (a generation run repeats one geometry): the two resize tables, their rows
    packed for the kernel, and the LDS the kernel takes.  The tensors are shared between the calls that hit the cache: read, not written."""
    l, r, t, b = pad
    geo = dict(bg_y=resize_taps(H + t + b, H, antialias), bg_x=resize_taps(W + l + r, W, antialias))
    geo["rows"] = np.concatenate([_rows(geo[key]).reshape(-1) for key in ("bg_y", "bg_x")])
    geo["lds_bytes"] = lds_bytes(dict(geo, H=H, W=W, bg_pad=pad, taps=torch.empty((1, 3, 3, k))))
    return geo


def lower_pyramid(H, W, n_fg, n_bg, bg_index, fg_index=None, *, blur, bg_pad=16, antialias=False):
    """A call as the tables the kernel reads (host arithmetic only; nothing is launched and the arguments are left untouched): a dict of
    fg_index, bg_index (B,) int32; taps (B,3,3,k) float32, [frame][plane kind][level]; bg_y, bg_x, each ``resize_taps`` of the padded axis;
    the sizes; lds_bytes; and ``params``, all of it packed as MMPyramidDesc.params wants it (int32 words, floats by their bits).
    Raises ValueError for what the kernel refuses: see ``pyramid_frames``."""
    low, fgi, bgi, taps = _lower_common(H, W, n_fg, n_bg, bg_index, fg_index, bg_pad, taps=lambda B: _taps(blur, B))
    H, W, pad = low["H"], low["W"], low["bg_pad"]
    k = taps.shape[-1]
    if k // 2 >= min(H, W):
        raise ValueError("a blur radius must be smaller than the dimension it reflects in: kernel %d on %d x %d" % (k, H, W))
    geo = _geometry(H, W, pad, k, bool(antialias))
    if geo["lds_bytes"] > LDS_BYTES:
        raise ValueError("the call takes %d bytes of LDS, more than %d: a smaller kernel, pad or image" % (geo["lds_bytes"], LDS_BYTES))
    low.update(antialias=bool(antialias), taps=taps, bg_y=geo["bg_y"], bg_x=geo["bg_x"], lds_bytes=geo["lds_bytes"])
    low["params"] = torch.from_numpy(np.concatenate([fgi, bgi, taps.numpy().view(np.int32).reshape(-1), geo["rows"]]))
    return low


def pyramid_frames(renders, backgrounds, bg_index, *, fg_index=None, blur, bg_pad=16, antialias=False, rounding="trunc", as_float=False):
    """Frames of the three-level pyramid blend as 8-bit pixels, all in one launch: (...,H,W,3) uint8, the dimensions of ``bg_index`` in front.

        bg0 = resize(reflection_pad(background));  v1, v2, v3 = blur(v0), blur(v1), blur(v2) for the mask m, bg and the render obj
        out = bg3*(1-m3) + obj3*m3 + (bg1-bg2)*(1-m2) + (obj1-obj2)*m2 + (bg0-bg1)*(1-m1) + (obj0-obj1)*m1

    renders, backgrounds, bg_index, fg_index, bg_pad, antialias, rounding, as_float
                 exactly as in ``composite_frames``: float (...,4,H,W) renders with the mask in channel 3, dense NCHW or NHWC memory read in
                 place, leading dimensions kept; float (n_bg,3|4,H,W) backgrounds; the background (and, with fg_index, the render) of each
                 frame; the reflection pad as an int or (left, right, top, bottom), resized back to (H,W) -- here with no blur before the
                 resize --; as_float gives the quantised values as (...,3,H,W) float32 ``q / 255``.
    blur         ``(kernel_size, sigma)`` -- sigma a float or a (frames,3,3) array indexed [frame][plane kind][level], the kinds being
                 mask, background, render: the order in which the reference draws its nine sigmas per frame, so
                 ``draw_sigmas(9 * n).view(n, 3, 3)`` draws them -- or ready taps (k,), (3,3,k) or (frames,3,3,k).  Every blur reflects at
                 the image's own edge; k odd, at most 15; a one-tap kernel makes a level the identity.

    The sums leave [0, 1], where the reference's ``np.uint8`` is undefined: the quantiser saturates and sends NaN to 0, as ``export_images``
    does.  ``PRESETS`` / ``preset`` hold the call site.  ValueError: mismatched shapes, an index outside its range, an even kernel or one
    above 15, a sigma or taps of another shape, a reflection pad or blur radius not smaller than the dimension it reflects in,
    more LDS than the chip has, an unknown rounding.  Not differentiable; the inputs are left unmodified; bitwise reproducible.

        frames = pyramid_frames(pred, Xa, torch.randint(0, B, (B,)), **preset("tool/generate_market_test", B))
        for f in frames.cpu().numpy(): PIL.Image.fromarray(f).save(...)                 # ONE device-to-host copy"""
    _, H, W, n_fg, shape = _check_inputs(renders, backgrounds, bg_index, fg_index, rounding)
    low = lower_pyramid(H, W, n_fg, backgrounds.shape[0], bg_index, fg_index, blur=blur, bg_pad=bg_pad, antialias=antialias)
    d = N.MMPyramidDesc()
    d.k = low["taps"].shape[-1]
    return _launch(d, "mm_pyramid_frames", low, renders, backgrounds, shape, H, W, rounding, as_float)
