"""Renders as 8-bit frames and contact sheets: host side of ``mm_export_images / mm_export_grid`` (csrc/mm_export.hip).

What the reference's evaluation and visualisation code does on the host after every render -- ``to_pil_image(X[i, :3].cpu())``,
``make_grid(X[:, :3])`` + ``permute`` + ``(image * 255.0).astype(np.uint8)``, ``save_image`` (trainer.py:546-769, test*.py) -- as one
launch on the device: each render pixel is read once (16 bytes, the renders' NHWC memory as it is) and 3 or 1 bytes are written, so
a quarter of the bytes cross to the host, in one copy.

The quantiser, every step rounded in fp32:

    rounding="trunc"     q = x * 255               to_pil_image's ``pic.mul(255).byte()``, numpy's ``(image * 255.0).astype(np.uint8)``
    rounding="nearest"   q = (x * 255) + 0.5       save_image's ``mul(255).add_(0.5).clamp_(0, 255).to(uint8)``

then NaN -> 0, clamp to [0, 255], convert toward zero.  For x in [0, 1] these are the reference's bytes.  Outside [0, 1] the reference's
cast is undefined (it wraps or not with the platform); this one SATURATES.  ``white=True`` first composes a 4-channel image over white
with its own alpha, ``x[:3] * m + (1 - m)`` with ``m = x[3:4]`` (trainer.py:755-757), like ``critic_inputs``' unmask 0.

``make_grid`` is restated from torchvision [recall-risk: torchvision is not installed where this was written; the arithmetic in
``grid_shape`` and DESIGN.md is from memory of torchvision.utils.make_grid and has not been run against it].  Nothing here is
differentiable.  Device tensors only."""
import torch

from . import _native as N

_CHANNELS = ("rgb", "mask", "rgba", "rgb+mask")
_ROUNDING = {"trunc": 0, "nearest": 1}


def _layout(x):
    """(tensor the kernel reads, its layout flag) for a (...,C,H,W) tensor: dense NCHW (0) and, for C = 4, dense NHWC (1: (...,H,W,4)
    memory, what ``render`` and ``render_views`` return) are read in place; anything else is copied"""
    if x.is_contiguous():
        return x, 0
    if x.shape[-3] == 4 and x.movedim(-3, -1).is_contiguous():
        return x, 1
    return x.contiguous(), 0


def _check(x, rounding, white, ranks, what):
    if not torch.is_tensor(x) or not x.dtype.is_floating_point:
        raise ValueError("x must be a float tensor, got %s" % (x.dtype if torch.is_tensor(x) else type(x)))
    if x.dim() not in ranks or x.shape[-3] not in (3, 4) or min(x.shape) < 1:
        raise ValueError("x must have shape %s with C 3 or 4, got %s" % (what, tuple(x.shape)))
    if rounding not in _ROUNDING:
        raise ValueError("rounding must be 'trunc' or 'nearest', got %r" % (rounding,))
    if white and x.shape[-3] != 4:
        raise ValueError("white=True needs the alpha of a 4-channel image, x has shape %s" % (tuple(x.shape),))


def _desc(x, B, Nv, rounding, white):
    x = x.detach()
    x, flag = _layout(x if x.dtype == torch.float32 else x.float())
    d = N.MMExportDesc()
    d.B, d.N, d.C, d.H, d.W = B, Nv, x.shape[-3], x.shape[-2], x.shape[-1]
    d.nhwc, d.rounding, d.white, d.x = flag, _ROUNDING[rounding], int(bool(white)), N.ptr(x)
    return d, x


def export_images(x, channels="rgb", rounding="trunc", white=False, as_float=False):
    """The images of a float (...,C,H,W) tensor, C 3 or 4, as 8-bit pixels; the leading dimensions are kept.

    channels: "rgb" -> (...,H,W,3) uint8; "mask" -> (...,H,W) uint8 from channel 3; "rgba" -> (...,H,W,4) uint8; "rgb+mask" -> the pair
    (rgb, mask) from one launch and one read of x.  All but "rgb" need C = 4.
    rounding, white: the module docstring has the quantiser and the composite over white (which changes rgb, never the mask).
    as_float: the same quantised values as float32 ``q / 255`` in planes -- (...,3,H,W), (...,H,W), (...,4,H,W): what ``to_tensor`` of the
    saved file gives, ready for ``ssim`` / ``recon_scores`` (the reference scores 8-bit images, trainer.py:550-559).

    Dense NCHW and, for C = 4, dense NHWC memory (a ``render`` or ``render_views`` result) are read in place; other strides go through
    ``.contiguous()``, other float dtypes through ``.float()``.  x is detached and left unmodified; the outputs are fresh device tensors:

        rgb, mask = export_images(dr.render_views(...)[0], "rgb+mask")     # (B,N,H,W,3), (B,N,H,W)
        frames = rgb.cpu().numpy()                                         # ONE device-to-host copy, a quarter of the float bytes
        PIL.Image.fromarray(frames[b, n]).save(...)                        # mode RGB; a mask is mode L"""
    _check(x, rounding, white, range(3, 65), "(...,C,H,W)")
    if channels not in _CHANNELS:
        raise ValueError("channels must be one of %s, got %r" % (", ".join(_CHANNELS), channels))
    if channels != "rgb" and x.shape[-3] != 4:
        raise ValueError("channels=%r needs a 4-channel image, x has shape %s" % (channels, tuple(x.shape)))
    N.require_device(x)
    lead, (H, W) = tuple(x.shape[:-3]), x.shape[-2:]
    n = 1
    for s in lead:
        n *= s
    d, x = _desc(x, n, 1, rounding, white)
    d.as_float = int(bool(as_float))
    dt = torch.float32 if as_float else torch.uint8
    shapes = {"rgb": lead + ((3, H, W) if as_float else (H, W, 3)), "mask": lead + (H, W), "rgba": lead + ((4, H, W) if as_float else (H, W, 4))}
    outs = {k: torch.empty(shapes[k], dtype=dt, device=x.device) for k in channels.split("+")}
    d.out_rgb, d.out_mask, d.out_rgba = N.ptr(outs.get("rgb")), N.ptr(outs.get("mask")), N.ptr(outs.get("rgba"))
    N.call("mm_export_images", x.device, d)
    return (outs["rgb"], outs["mask"]) if channels == "rgb+mask" else outs[channels]


def grid_shape(B, H, W, nrow=8, padding=2):
    """(Hg, Wg) of ``make_grid`` for B images of H x W (host arithmetic only) [recall-risk: restated from torchvision, see the module
    docstring]: one image is the sheet itself; otherwise xmaps = min(nrow, B) columns and ymaps = ceil(B / xmaps) rows of cells of
    (H + padding) x (W + padding), image k = y * xmaps + x at the bottom right of its cell, and one more gutter at the bottom and right."""
    B, H, W, nrow, padding = int(B), int(H), int(W), int(nrow), int(padding)
    if B < 1 or H < 1 or W < 1:
        raise ValueError("B, H and W must be positive, got %r" % ((B, H, W),))
    if nrow < 1:
        raise ValueError("nrow must be at least 1, got %r" % (nrow,))
    if padding < 0:
        raise ValueError("padding must not be negative, got %r" % (padding,))
    if B == 1:
        return H, W
    xmaps = min(nrow, B)
    ymaps = -(-B // xmaps)
    return (H + padding) * ymaps + padding, (W + padding) * xmaps + padding


def export_grid(x, nrow=8, padding=2, pad_value=0.0, rounding="trunc", white=False):
    """Contact sheets of a float batch as 8-bit HWC frames: (B,C,H,W) -> (Hg,Wg,3) uint8, (B,N,C,H,W) -> (N,Hg,Wg,3) uint8 with frame n
    = ``make_grid(x[:, n, :3], nrow, padding, pad_value)`` permuted to HWC and quantised -- all N frames in one launch, e.g. the 36
    frames of a turntable from one ``render_views`` result (trainer.py:616-631).  ``grid_shape`` has (Hg, Wg); the gutters and the
    empty cells of a short last row hold the quantised ``pad_value``.  rounding, white, layouts and dtypes as in ``export_images``.

        sheet = export_grid(frames)                                        # (36,Hg,Wg,3), on the device; encode_gif(sheet).write(path)"""
    _check(x, rounding, white, (4, 5), "(B,C,H,W) or (B,N,C,H,W)")
    B, Nv = x.shape[0], (x.shape[1] if x.dim() == 5 else 1)
    Hg, Wg = grid_shape(B, x.shape[-2], x.shape[-1], nrow, padding)
    N.require_device(x)
    five = x.dim() == 5
    d, x = _desc(x, B, Nv, rounding, white)
    d.nrow, d.padding, d.pad_value = int(nrow), int(padding), float(pad_value)
    out = torch.empty(((Nv,) if five else ()) + (Hg, Wg, 3), dtype=torch.uint8, device=x.device)
    d.out_grid = N.ptr(out)
    N.call("mm_export_grid", x.device, d)
    return out
