"""Renders composed over blurred backgrounds as 8-bit frames: host side of ``mm_composite_frames`` (csrc/mm_composite.hip).

What the reference's dataset-generation scripts do on the host, one image at a time, after every render (generate_market++.py:308-349,
generate_market_new_class9.py:323-347, tool/generate_market.py:293-313) -- ``makeup_hole``, ``GaussianBlur`` of the mask,
``ReplicationPad2d`` + ``Resize``, ``ReflectionPad2d`` + ``GaussianBlur`` + ``Resize`` of a random background, the blend and
``np.uint8(x * 255)`` behind a blocking ``.cpu()`` -- as ONE launch for all the frames of a batch, and one byte-sized copy to the host.

The host lowers a call to small tables (``lower_composite``); no transcendental runs on the device:

    gaussian_taps   torchvision's 1-D Gaussian kernel [recall-risk: torchvision is not installed where this was written; the arithmetic
                    is from memory of torchvision.transforms.functional's _get_gaussian_kernel1d and has not been run against it]
    resize_taps     torch's bilinear resize with align_corners=False along one axis, with and without antialias (pinned to live
                    ``F.interpolate`` by tests/test_composite_host.py)

The device then runs, per frame and in fp32 with every operation rounded as written and every sum in ascending tap order from 0: the
hole fill, the separable blur (x, then y; reflect border) and the replicate pad + separable resize (x, then y) of the mask; the
reflection pad (index arithmetic), separable blur and resize of the background; ``fg * m + bg * (1 - m)``; ``export_images``' quantiser.
DESIGN.md has the order in full.  The blur is separable where torchvision convolves with the outer product, and the resize is
separable where torch's two-tap bilinear is one 2x2 expression: the results differ from the functional composition by rounding only
(within 1e-5; bytes differ by one only where ``x * 255`` lies within 2e-3 of an integer).

Out of scope: reproducing the reference's random streams (the caller draws ``bg_index`` and the sigmas: ``draw_sigmas``); gradients.  JPEG encoding: ``encode_jpeg`` (jpeg.py).
tool/generate_market_test.py's three-level pyramid blend and its resize-before-blur order: ``pyramid_frames`` (pyramid.py).  Device tensors only."""
import functools

import numpy as np
import torch

from . import _native as N
from .frames import (LDS_BYTES, MAX_KERNEL, MAX_TAPS, ROW_WORDS, ROWS, _check_inputs, _index, _launch, _lower_common, _pad4, _rows,  # noqa: F401
                     band_bytes_lds, draw_sigmas, gaussian_taps, resize_taps)      # (the table builders live in frames.py; their names stay importable from here)

# the three call sites; a sigma of None is drawn per frame (draw_sigmas), as GaussianBlur(k) without sigma draws it per call
PRESETS = {
    "generate_market++": dict(fill_holes=True, mask_blur=(5, 3.0), mask_pad=3, bg_pad=(8, 8, 16, 16), bg_blur=(5, None)),
    "generate_market_new_class9": dict(fill_holes=False, mask_blur=(7, None), mask_pad=0, bg_pad=16, bg_blur=(7, None)),
    "tool/generate_market": dict(fill_holes=False, mask_blur=(31, 2.0), mask_pad=0, bg_pad=16, bg_blur=(31, 2.0)),
}


def preset(name, n, generator=None):
    """The keyword arguments of ``composite_frames`` for one of the reference's call sites (``PRESETS``) and n frames, the sigmas the
    call site leaves to ``GaussianBlur`` drawn per frame: one draw for the mask and one for the background."""
    kw = dict(PRESETS[name])
    for key in ("mask_blur", "bg_blur"):
        k, sigma = kw[key]
        kw[key] = (k, draw_sigmas(n, generator=generator) if sigma is None else sigma)
    return kw


@functools.lru_cache(maxsize=32)
def _gaussian_taps_fixed(k, sigma):
    return gaussian_taps(k, torch.tensor(sigma, dtype=torch.float32))


def _taps(blur, n, what):
    """(n,k) float32 taps of a blur argument: None (no blur: one tap of 1), (kernel_size, sigma), or ready taps (k,) / (n,k)"""
    if blur is None:
        return torch.ones((n, 1), dtype=torch.float32)
    if isinstance(blur, tuple) and len(blur) == 2 and not torch.is_tensor(blur[0]) and np.ndim(blur[0]) == 0:
        t = _gaussian_taps_fixed(int(blur[0]), float(blur[1])) if isinstance(blur[1], (int, float)) else gaussian_taps(*blur)
    else:
        t = torch.as_tensor(blur, dtype=torch.float32).detach().cpu()
    if t.dim() == 1:
        t = t[None].expand(n, -1)
    if t.dim() != 2 or t.shape[0] != n or t.shape[1] < 1 or t.shape[1] > MAX_KERNEL or t.shape[1] % 2 == 0:
        raise ValueError("%s must be (kernel_size, sigma) or taps of shape (k,) or (%d,k) with k odd and at most %d, got %s"
                         % (what, n, MAX_KERNEL, tuple(t.shape)))
    return t.contiguous()


def _band_rows(start, count, y0, y1, p, Hv):
    lo, hi = int(start[y0:y1].min()), int((start[y0:y1] + count[y0:y1]).max())
    c_lo = min(max(lo - p, 0), Hv - 1)
    return c_lo, min(max(hi - 1 - p, 0), Hv - 1) - c_lo + 1


def lds_bytes(low):
    """bytes of LDS the kernel takes for a lowered call (include/mm_render.h, MMCompositeDesc): mm::composite_lds_bytes in Python"""
    H, W = low["H"], low["W"]
    l, r, t, b = low["bg_pad"]
    cap = 0
    for y0 in range(0, H, ROWS):
        y1 = min(y0 + ROWS, H)
        n = _band_rows(low["mask_y"][0].numpy(), low["mask_y"][1].numpy(), y0, y1, low["mask_pad"], H)[1]
        cap = max(cap, (n + low["mask_taps"].shape[1] - 1) * W)
        n = _band_rows(low["bg_y"][0].numpy(), low["bg_y"][1].numpy(), y0, y1, 0, H + t + b)[1]
        cap = max(cap, (n + low["bg_taps"].shape[1] - 1) * (W + l + r))
    cap = (cap + 3) // 4 * 4
    return 4 * (2 * cap + (ROWS * W + 3) // 4 * 4) + band_bytes_lds(W)


@functools.lru_cache(maxsize=32)
def _geometry(H, W, mask_pad, pad, km, kb, antialias):
    """what a call's sizes alone decide, kept between calls (a generation run repeats one geometry): the four resize tables, their rows
    packed for the kernel, and the LDS the kernel takes.  The tensors are shared between the calls that hit the cache: read, not written."""
    l, r, t, b = pad
    geo = dict(mask_y=resize_taps(H + 2 * mask_pad, H, antialias), mask_x=resize_taps(W + 2 * mask_pad, W, antialias),
               bg_y=resize_taps(H + t + b, H, antialias), bg_x=resize_taps(W + l + r, W, antialias))
    geo["rows"] = np.concatenate([_rows(geo[k]).reshape(-1) for k in ("mask_y", "mask_x", "bg_y", "bg_x")])
    geo["lds_bytes"] = lds_bytes(dict(geo, H=H, W=W, mask_pad=mask_pad, bg_pad=pad, mask_taps=torch.empty((1, km)), bg_taps=torch.empty((1, kb))))
    return geo


def lower_composite(H, W, n_fg, n_bg, bg_index, fg_index=None, mask_blur=None, mask_pad=0, bg_pad=0, bg_blur=None, antialias=False):
    """A call as the tables the kernel reads (host arithmetic only; nothing is launched and the arguments are left untouched): a dict of
    fg_index, bg_index (B,) int32; mask_taps (B,km), bg_taps (B,kb) float32; mask_y, mask_x, bg_y, bg_x, each ``resize_taps`` of the
    padded axis; the sizes; and ``params``, all of it packed as MMCompositeDesc.params wants it (int32 words, floats by their bits).
    Raises ValueError for what the kernel refuses: see ``composite_frames``."""
    mask_pad = int(mask_pad)
    low, fgi, bgi, (mt, bt) = _lower_common(H, W, n_fg, n_bg, bg_index, fg_index, bg_pad, mask_pad=mask_pad,
                                            taps=lambda B: (_taps(mask_blur, B, "mask_blur"), _taps(bg_blur, B, "bg_blur")))
    H, W, (l, r, t, b) = low["H"], low["W"], low["bg_pad"]
    Hp, Wp = H + t + b, W + l + r
    if mt.shape[1] // 2 >= min(H, W) or bt.shape[1] // 2 >= min(Hp, Wp):
        raise ValueError("a blur radius must be smaller than the dimension it reflects in: kernels %d, %d on %d x %d, %d x %d"
                         % (mt.shape[1], bt.shape[1], H, W, Hp, Wp))
    geo = _geometry(H, W, mask_pad, low["bg_pad"], mt.shape[1], bt.shape[1], bool(antialias))
    if geo["lds_bytes"] > LDS_BYTES:
        raise ValueError("the call takes %d bytes of LDS, more than %d: a smaller kernel, pad or image" % (geo["lds_bytes"], LDS_BYTES))
    low.update(mask_pad=mask_pad, antialias=bool(antialias), mask_taps=mt, bg_taps=bt, mask_y=geo["mask_y"], mask_x=geo["mask_x"], bg_y=geo["bg_y"], bg_x=geo["bg_x"])
    low["params"] = torch.from_numpy(np.concatenate([fgi, bgi, mt.numpy().view(np.int32).reshape(-1), bt.numpy().view(np.int32).reshape(-1), geo["rows"]]))
    return low


def composite_frames(renders, backgrounds, bg_index, *, fg_index=None, fill_holes=False, mask_blur=None, mask_pad=0, bg_pad=0,
                     bg_blur=None, antialias=False, rounding="trunc", as_float=False):
    """Frames ``fg * m' + bg' * (1 - m')`` as 8-bit pixels, all in one launch: (...,H,W,3) uint8, the dimensions of ``bg_index`` in front.

    renders      float (...,4,H,W): rgb and the mask m in channel 3.  Dense NCHW and dense NHWC memory (a ``render`` or ``render_views``
                 result) are read in place, anything else through ``.contiguous()``; the leading dimensions are kept.
    backgrounds  float (n_bg,3|4,H,W), e.g. the input batch ``Xa`` itself: channels 0-2 are read, no ``Xa[:, :3]`` copy.
    bg_index     integers of shape ``renders.shape[:-3]`` (of ``fg_index``'s shape if that is given): the background of each frame,
                 what the reference draws with ``random.randint(0, B - 1)``.
    fg_index     the render of each frame, flat over the leading dimensions (default: frame o is render o) -- generate_market++'s
                 ``diff_indices[:B // 2]``.
    fill_holes   ``makeup_hole``: 3x3 mean with zero padding, > 0.7 -> 1, <= 0.7 -> 0 (NaN stays).
    mask_blur, bg_blur   None, ``(kernel_size, sigma)`` -- sigma a float or one per frame, see ``draw_sigmas`` -- or ready taps (k,) /
                 (frames,k); reflect border; k odd, at most 31.
    mask_pad     p > 0: the blurred mask is replicate-padded by p and resized back to (H,W).
    bg_pad       reflection pad of the background, an int or (left, right, top, bottom), before its blur; resized back to (H,W) after.
    antialias    of both resizes (False: tensors under torchvision 0.12; True: current torchvision).
    rounding, as_float   ``export_images``' quantiser, unchanged; as_float gives the quantised values as (...,3,H,W) float32 ``q / 255``.

    ``PRESETS`` / ``preset`` hold the three call sites.  ValueError: mismatched shapes, an index outside its range, an even kernel or one
    above 31, a reflection pad or blur radius not smaller than the dimension it reflects in, more than 8 resize taps, more LDS than the
    chip has, an unknown rounding.  Not differentiable; the inputs are left unmodified; bitwise reproducible.

        frames = composite_frames(pred, Xa, torch.randint(0, B, (B,)), **preset("generate_market++", B))
        for f in frames.cpu().numpy(): PIL.Image.fromarray(f).save(...)                 # ONE device-to-host copy"""
    _, H, W, n_fg, shape = _check_inputs(renders, backgrounds, bg_index, fg_index, rounding)
    low = lower_composite(H, W, n_fg, backgrounds.shape[0], bg_index, fg_index, mask_blur, mask_pad, bg_pad, bg_blur, antialias)
    d = N.MMCompositeDesc()
    d.fill_holes, d.mask_k, d.bg_k, d.mask_pad = int(bool(fill_holes)), low["mask_taps"].shape[1], low["bg_taps"].shape[1], low["mask_pad"]
    return _launch(d, "mm_composite_frames", low, renders, backgrounds, shape, H, W, rounding, as_float)
