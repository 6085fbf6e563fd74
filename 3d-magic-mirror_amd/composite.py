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
import ctypes
import functools

import numpy as np
import torch

from . import _native as N
from .export import _ROUNDING, _layout

ROWS = 8                # MM_COMPOSITE_ROWS
MAX_KERNEL = 31         # MM_COMPOSITE_MAX_KERNEL
MAX_TAPS = 8            # MM_COMPOSITE_MAX_TAPS
ROW_WORDS = 10          # MM_COMPOSITE_ROW_WORDS
LDS_BYTES = 160 * 1024

# the three call sites; a sigma of None is drawn per frame (draw_sigmas), as GaussianBlur(k) without sigma draws it per call
PRESETS = {
    "generate_market++": dict(fill_holes=True, mask_blur=(5, 3.0), mask_pad=3, bg_pad=(8, 8, 16, 16), bg_blur=(5, None)),
    "generate_market_new_class9": dict(fill_holes=False, mask_blur=(7, None), mask_pad=0, bg_pad=16, bg_blur=(7, None)),
    "tool/generate_market": dict(fill_holes=False, mask_blur=(31, 2.0), mask_pad=0, bg_pad=16, bg_blur=(31, 2.0)),
}


def draw_sigmas(n, low=0.1, high=2.0, generator=None):
    """n sigmas as ``GaussianBlur(k)`` draws them, one per call, uniform in [low, high): (n,) float32.  (Not the reference's stream.)"""
    return torch.empty(int(n), dtype=torch.float32).uniform_(float(low), float(high), generator=generator)


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


def gaussian_taps(kernel_size, sigma):
    """torchvision's 1-D Gaussian kernel [recall-risk, see the module docstring]: x = linspace(-(k-1)/2, (k-1)/2, k),
    exp(-0.5 (x / sigma)^2), divided by its sum, in float32.  sigma a float -> (k,); a (B,) sequence -> (B,k), one row per frame."""
    k = int(kernel_size)
    if k < 1 or k > MAX_KERNEL or k % 2 == 0:
        raise ValueError("kernel_size must be odd and in [1, %d], got %r" % (MAX_KERNEL, kernel_size))
    sig = torch.as_tensor(sigma, dtype=torch.float32)
    if sig.dim() > 1 or not bool((sig > 0).all()):
        raise ValueError("sigma must be a positive float or a (B,) sequence of them, got %r" % (sigma,))
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / sig[..., None]).pow(2))
    return pdf / pdf.sum(-1, keepdim=True)


def resize_taps(n_in, n_out, antialias=False):
    """One axis of torch's bilinear resize with align_corners=False as taps: (start (n_out,) int32, count (n_out,) int32, weights
    (n_out, MAX_TAPS) float32, zero beyond count); output i = sum_t weights[i, t] * input[start[i] + t].

    antialias=False (tensors under torchvision 0.12): src = max(scale (i + 0.5) - 0.5, 0), taps floor(src) and the next, weights
    1 - l and l.  antialias=True (current torchvision): the triangle filter of support max(scale, 1) around scale (i + 0.5),
    normalised.  Taps of weight 0 at either end are dropped (so n_in == n_out is the identity, one tap of 1); more than MAX_TAPS taps
    -- an antialiased ratio beyond 3.5 -- are refused."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("n_in and n_out must be positive, got %r" % ((n_in, n_out),))
    i = np.arange(n_out)
    if not antialias:
        scale = np.float32(n_in) / np.float32(n_out)
        src = np.maximum(scale * (i.astype(np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        lam = (src - i0.astype(np.float32)).astype(np.float64)
        lam = np.where(i0 + 1 > n_in - 1, 0.0, np.clip(lam, 0.0, 1.0))
        start, size = i0, np.full(n_out, 2)
        w = np.zeros((n_out, 2))
        w[:, 0], w[:, 1] = 1.0 - lam, lam
    else:
        scale = n_in / n_out
        support = scale if scale >= 1.0 else 1.0
        inv = 1.0 / scale if scale >= 1.0 else 1.0
        center = scale * (i + 0.5)
        start = np.maximum((center - support + 0.5).astype(np.int64), 0)
        size = np.minimum((center + support + 0.5).astype(np.int64), n_in) - start
        j = np.arange(int(size.max()))
        w = np.maximum(0.0, 1.0 - np.abs((j[None] + start[:, None] - center[:, None] + 0.5) * inv))
        w = np.where(j[None] < size[:, None], w, 0.0)
        w = w / w.sum(1, keepdims=True)
    # drop the taps of weight 0 at either end
    nz = w != 0
    first = nz.argmax(1)
    last = w.shape[1] - 1 - nz[:, ::-1].argmax(1)
    count = last - first + 1
    if int(count.max()) > MAX_TAPS:
        raise ValueError("resize %d -> %d takes %d taps per output, more than %d: an antialiased ratio cap of 3.5" % (n_in, n_out, int(count.max()), MAX_TAPS))
    out = np.zeros((n_out, MAX_TAPS), dtype=np.float32)
    for t in range(int(count.max())):
        col = np.minimum(first + t, w.shape[1] - 1)
        out[:, t] = np.where(t < count, w[i, col], 0.0)
    return (torch.from_numpy((start + first).astype(np.int32)), torch.from_numpy(count.astype(np.int32)), torch.from_numpy(out))


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


def _pad4(bg_pad):
    p = (int(bg_pad),) * 4 if np.ndim(bg_pad) == 0 else tuple(int(v) for v in bg_pad)
    if len(p) != 4:
        raise ValueError("bg_pad must be an int or (left, right, top, bottom), got %r" % (bg_pad,))
    return p


def _index(idx, n, what):
    a = np.asarray(idx.detach().cpu() if torch.is_tensor(idx) else idx)
    if a.dtype.kind not in "iu":
        raise ValueError("%s must hold integers, got %s" % (what, a.dtype))
    if a.size and (int(a.min()) < 0 or int(a.max()) >= n):
        raise ValueError("%s outside [0, %d)" % (what, n))
    return a.astype(np.int32)


def _rows(table):
    start, count, w = table
    r = np.empty((start.shape[0], ROW_WORDS), dtype=np.int32)
    r[:, 0], r[:, 1] = start.numpy(), count.numpy()
    r[:, 2:] = w.numpy().view(np.int32)
    return r


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
    return 4 * (2 * cap + (ROWS * W + 3) // 4 * 4) + (ROWS * W * 3 + 16 + 15) // 16 * 16


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
    H, W, n_fg, n_bg, mask_pad = int(H), int(W), int(n_fg), int(n_bg), int(mask_pad)
    if H < 1 or W < 1 or n_fg < 1 or n_bg < 1:
        raise ValueError("H, W and the numbers of renders and backgrounds must be positive, got %r" % ((H, W, n_fg, n_bg),))
    bgi = _index(bg_index, n_bg, "bg_index").reshape(-1)
    fgi = np.arange(n_fg, dtype=np.int32) if fg_index is None else _index(fg_index, n_fg, "fg_index").reshape(-1)
    if fgi.shape != bgi.shape or bgi.size < 1:
        raise ValueError("fg_index and bg_index must name the same, positive number of frames, got %d and %d" % (fgi.size, bgi.size))
    B = bgi.size
    mt, bt = _taps(mask_blur, B, "mask_blur"), _taps(bg_blur, B, "bg_blur")
    l, r, t, b = pad = _pad4(bg_pad)
    if mask_pad < 0 or min(pad) < 0:
        raise ValueError("pads must not be negative, got mask_pad %d, bg_pad %r" % (mask_pad, pad))
    if max(l, r) >= W or max(t, b) >= H:
        raise ValueError("a reflection pad must be smaller than the dimension it reflects in: bg_pad %r on %d x %d" % (pad, H, W))
    Hp, Wp = H + t + b, W + l + r
    if mt.shape[1] // 2 >= min(H, W) or bt.shape[1] // 2 >= min(Hp, Wp):
        raise ValueError("a blur radius must be smaller than the dimension it reflects in: kernels %d, %d on %d x %d, %d x %d"
                         % (mt.shape[1], bt.shape[1], H, W, Hp, Wp))
    geo = _geometry(H, W, mask_pad, pad, mt.shape[1], bt.shape[1], bool(antialias))
    if geo["lds_bytes"] > LDS_BYTES:
        raise ValueError("the call takes %d bytes of LDS, more than %d: a smaller kernel, pad or image" % (geo["lds_bytes"], LDS_BYTES))
    low = dict(B=B, H=H, W=W, n_fg=n_fg, n_bg=n_bg, mask_pad=mask_pad, bg_pad=pad, antialias=bool(antialias),
               fg_index=torch.from_numpy(fgi.copy()), bg_index=torch.from_numpy(bgi.copy()), mask_taps=mt, bg_taps=bt,
               mask_y=geo["mask_y"], mask_x=geo["mask_x"], bg_y=geo["bg_y"], bg_x=geo["bg_x"])
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
    for x, what, ok in ((renders, "renders", lambda s: len(s) >= 3 and s[-3] == 4), (backgrounds, "backgrounds", lambda s: len(s) == 4 and s[1] in (3, 4))):
        if not torch.is_tensor(x) or not x.dtype.is_floating_point:
            raise ValueError("%s must be a float tensor, got %s" % (what, x.dtype if torch.is_tensor(x) else type(x)))
        if not ok(tuple(x.shape)) or min(x.shape) < 1:
            raise ValueError("%s must have shape %s, got %s" % (what, "(...,4,H,W)" if what == "renders" else "(n_bg,3|4,H,W)", tuple(x.shape)))
    if tuple(backgrounds.shape[-2:]) != tuple(renders.shape[-2:]):
        raise ValueError("renders and backgrounds must have the same H x W, got %s and %s" % (tuple(renders.shape), tuple(backgrounds.shape)))
    if rounding not in _ROUNDING:
        raise ValueError("rounding must be 'trunc' or 'nearest', got %r" % (rounding,))
    lead, (H, W) = tuple(renders.shape[:-3]), renders.shape[-2:]
    n_fg = int(np.prod(lead, dtype=np.int64))
    shape = tuple(np.shape(bg_index if fg_index is None else fg_index))
    if tuple(np.shape(bg_index)) != shape or (fg_index is None and shape != lead):
        raise ValueError("bg_index must have the shape of %s, got %s" % ("fg_index, %s" % (shape,) if fg_index is not None else
                                                                         "the renders' leading dimensions, %s" % (lead,), tuple(np.shape(bg_index))))
    low = lower_composite(H, W, n_fg, backgrounds.shape[0], bg_index, fg_index, mask_blur, mask_pad, bg_pad, bg_blur, antialias)
    N.require_device(renders, backgrounds)
    fg = renders.detach()
    fg, flag = _layout(fg if fg.dtype == torch.float32 else fg.float())
    bg = backgrounds.detach()
    bg = (bg if bg.dtype == torch.float32 else bg.float()).contiguous()
    B = low["B"]
    host = torch.empty(low["params"].shape, dtype=torch.int32, pin_memory=True)
    host.copy_(low["params"])
    dev = host.to(fg.device, non_blocking=True)
    out = torch.empty(shape + ((3, H, W) if as_float else (H, W, 3)), dtype=torch.float32 if as_float else torch.uint8, device=fg.device)
    d = N.MMCompositeDesc()
    d.B, d.H, d.W, d.n_fg, d.n_bg, d.bg_C = B, H, W, n_fg, bg.shape[0], bg.shape[1]
    d.fg_nhwc, d.fill_holes, d.mask_k, d.bg_k, d.mask_pad = flag, int(bool(fill_holes)), low["mask_taps"].shape[1], low["bg_taps"].shape[1], low["mask_pad"]
    d.bg_pad = (ctypes.c_int32 * 4)(*low["bg_pad"])
    d.rounding, d.as_float = _ROUNDING[rounding], int(bool(as_float))
    d.renders, d.backgrounds, d.params_host, d.params, d.out = N.ptr(fg), N.ptr(bg), ctypes.c_void_p(host.data_ptr()), N.ptr(dev), N.ptr(out)
    N.check(N.lib().mm_composite_frames(ctypes.byref(d), N.current_stream(fg.device)), "mm_composite_frames")
    return out
