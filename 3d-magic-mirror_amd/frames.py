"""What the frame makers share on the host: ``composite_frames`` (composite.py) and ``pyramid_frames`` (pyramid.py), whose kernels share
csrc/mm_frame.h.  The table builders -- ``gaussian_taps``, ``resize_taps`` and the packing of resize rows --, the validation of a call's
tensors and indices, the part of a lowering that both have (``_lower_common``) and the launch (``_launch``): layout and float handling, the
tables' upload from pinned memory, the output and the descriptor fields that MMCompositeDesc and MMPyramidDesc have in common."""
import ctypes

import numpy as np
import torch

from . import _native as N
from .export import _ROUNDING, _layout

ROWS = 8                # MM_COMPOSITE_ROWS, MM_PYRAMID_ROWS: output rows per workgroup
MAX_KERNEL = 31         # the largest blur any frame maker takes (MM_COMPOSITE_MAX_KERNEL): gaussian_taps' bound
MAX_TAPS = 8            # MM_COMPOSITE_MAX_TAPS, MM_PYRAMID_MAX_TAPS
ROW_WORDS = 10          # MM_COMPOSITE_ROW_WORDS, MM_PYRAMID_ROW_WORDS
LDS_BYTES = 160 * 1024


def draw_sigmas(n, low=0.1, high=2.0, generator=None):
    """n sigmas as ``GaussianBlur(k)`` draws them, one per call, uniform in [low, high): (n,) float32.  (Not the reference's stream.)"""
    return torch.empty(int(n), dtype=torch.float32).uniform_(float(low), float(high), generator=generator)


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


def resize_taps(n_in, n_out, antialias=False, coords=np.float32):
    """One axis of torch's bilinear resize with align_corners=False as taps: (start (n_out,) int32, count (n_out,) int32, weights
    (n_out, MAX_TAPS) float32, zero beyond count); output i = sum_t weights[i, t] * input[start[i] + t].

    antialias=False (tensors under torchvision 0.12): src = max(scale (i + 0.5) - 0.5, 0), taps floor(src) and the next, weights
    1 - l and l.  antialias=True (current torchvision): the triangle filter of support max(scale, 1) around scale (i + 0.5),
    normalised.  Taps of weight 0 at either end are dropped (so n_in == n_out is the identity, one tap of 1); more than MAX_TAPS taps
    -- an antialiased ratio beyond 3.5 -- are refused.

    coords (antialias=False): the type the source coordinate is formed in.  np.float32 is torch's fp32 kernel, whose coordinate carries the
    rounding of a number as large as n_in (1e-5 of a weight at n_in = 128); np.float64 is the resize of a float64 tensor, each weight
    then rounded to fp32 once (fid.py: its inputs are held to the float64 composition)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("n_in and n_out must be positive, got %r" % ((n_in, n_out),))
    i = np.arange(n_out)
    if not antialias:
        ct = np.dtype(coords).type
        scale = ct(n_in) / ct(n_out)
        src = np.maximum(scale * (i.astype(ct) + ct(0.5)) - ct(0.5), ct(0))
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        lam = (src - i0.astype(ct)).astype(np.float64)
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


def band_bytes_lds(W):
    """mm::frame_band_bytes_lds: LDS for the bytes of a band at any 16-byte phase"""
    return (ROWS * W * 3 + 16 + 15) // 16 * 16


def _check_inputs(renders, backgrounds, bg_index, fg_index, rounding):
    """The tensors, index shapes and rounding of a call: (lead, H, W, n_fg, shape), shape being the frames' leading dimensions"""
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
    return lead, H, W, n_fg, shape


def _lower_common(H, W, n_fg, n_bg, bg_index, fg_index, bg_pad, taps, mask_pad=None):
    """What every lowering begins with, in the order the refusals are raised: positive sizes, the two index tables, the frame count B,
    the kernel's own taps (``taps(B)``), the pads.  Returns the common entries of the lowered dict, the tables as arrays, and the taps."""
    H, W, n_fg, n_bg = int(H), int(W), int(n_fg), int(n_bg)
    if H < 1 or W < 1 or n_fg < 1 or n_bg < 1:
        raise ValueError("H, W and the numbers of renders and backgrounds must be positive, got %r" % ((H, W, n_fg, n_bg),))
    bgi = _index(bg_index, n_bg, "bg_index").reshape(-1)
    fgi = np.arange(n_fg, dtype=np.int32) if fg_index is None else _index(fg_index, n_fg, "fg_index").reshape(-1)
    if fgi.shape != bgi.shape or bgi.size < 1:
        raise ValueError("fg_index and bg_index must name the same, positive number of frames, got %d and %d" % (fgi.size, bgi.size))
    t = taps(bgi.size)
    l, r, top, b = pad = _pad4(bg_pad)
    if min(pad + (mask_pad or 0,)) < 0:
        raise ValueError("pads must not be negative, got %sbg_pad %r" % ("" if mask_pad is None else "mask_pad %d, " % mask_pad, pad))
    if max(l, r) >= W or max(top, b) >= H:
        raise ValueError("a reflection pad must be smaller than the dimension it reflects in: bg_pad %r on %d x %d" % (pad, H, W))
    low = dict(B=bgi.size, H=H, W=W, n_fg=n_fg, n_bg=n_bg, bg_pad=pad, fg_index=torch.from_numpy(fgi.copy()), bg_index=torch.from_numpy(bgi.copy()))
    return low, fgi, bgi, t


def _launch(desc, fn_name, low, fg, bg, shape, H, W, rounding, as_float):
    """Fill the fields the two descriptors share and call ``fn_name``: the renders in place where dense NCHW / NHWC, float32 otherwise;
    the tables through pinned memory; (shape,H,W,3) uint8 frames, or (shape,3,H,W) float32 with as_float."""
    N.require_device(fg, bg)
    fg = fg.detach()
    fg, desc.fg_nhwc = _layout(fg if fg.dtype == torch.float32 else fg.float())
    bg = bg.detach()
    bg = (bg if bg.dtype == torch.float32 else bg.float()).contiguous()
    host, dev = N.upload_int32(low["params"], fg.device)
    out = torch.empty(shape + ((3, H, W) if as_float else (H, W, 3)), dtype=torch.float32 if as_float else torch.uint8, device=fg.device)
    desc.B, desc.H, desc.W, desc.n_fg, desc.n_bg, desc.bg_C = low["B"], H, W, low["n_fg"], bg.shape[0], bg.shape[1]
    desc.bg_pad = (ctypes.c_int32 * 4)(*low["bg_pad"])
    desc.rounding, desc.as_float = _ROUNDING[rounding], int(bool(as_float))
    desc.renders, desc.backgrounds, desc.params_host, desc.params, desc.out = N.ptr(fg), N.ptr(bg), ctypes.c_void_p(host.data_ptr()), N.ptr(dev), N.ptr(out)
    N.call(fn_name, fg.device, desc)
    return out
