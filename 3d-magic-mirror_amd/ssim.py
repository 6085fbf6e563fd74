"""pytorch_msssim's ``ssim`` / ``ms_ssim`` / ``SSIM`` / ``MS_SSIM`` on the MI355X kernels (csrc/mm_ssim.hip behind ``mm_ssim_*``), and
``recon_scores`` / ``recon_scores_as_saved``, the reference's two evaluation numbers for a whole batch (of the tensors / of their saved JPEG files).

The reference scores every test reconstruction with ``pytorch_msssim.ssim(ori, rec, data_range=1)`` (trainer.py:771-795, 911-935;
test.py:428-457) and imports the package at module top (trainer.py:38, test.py:34).  Names, argument order and defaults here are
pytorch_msssim's; ``shim_eval/pytorch_msssim`` re-exports them under the package's own name.

Semantics, recalled (pytorch_msssim is not vendored; tools/mint_msssim_fixture.py pins them where it is installed):
  R1 window   coords = arange(size, float32) - size//2, g = exp(-coords^2 / (2 sigma^2)), g /= g.sum(), all in fp32.
  R2 filter   grouped, padding 0, along H first, then along W; a dimension with s < win_size is not filtered (upstream warns).
  R3 consts   C1 = (K1 data_range)^2, C2 = (K2 data_range)^2.
  R4 moments  sx2 = G*x^2 - mx^2, sy2 = G*y^2 - my^2, sxy = G*xy - mx my.
  R5 maps     cs_map = (2 sxy + C2) / (sx2 + sy2 + C2), ssim_map = (2 mx my + C1) / (mx^2 + my^2 + C1) * cs_map.
  R6 reduce   per channel: the mean over the valid spatial extent; size_average=True: the mean over (N,C); False: over C, shape (N,).
  R7 shapes   trailing singleton dims past dim 1 are squeezed; X and Y must have equal shapes.
  R8 nonnegative_ssim: relu on the per-channel ssim (torch.relu: a NaN stays NaN and its gradient passes).
  R9 ms_ssim  weights [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]; asserts min(H,W) > (win_size-1) 2^4; levels 1-4 take relu(cs) and
              then avg_pool2d(kernel 2, padding [s % 2 for s in spatial]); the last level takes relu(ssim per channel); the result is
              prod(stack ** weights), then the same mean.

Inputs are fp32 (N,C,H,W) with any strides (``ssim(rgbs[:, :3], gt[:, :3])`` on the renderer's NHWC-stored output reads it in place).
Host tensors are moved to the current HIP device and the result comes back on the host, as in ``ops.mask_iou``.  fp16 / bf16 and 5-D
(volumetric) inputs are refused.  ``ms_ssim`` is composed here from the SSIM op (which also returns cs) and ``F.avg_pool2d``.
"""
import functools
import warnings

import torch
import torch.nn.functional as F

from . import _native as N

MS_WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]


def _fspecial_gauss_1d(size, sigma):
    """R1: the (1,1,size) fp32 Gaussian window."""
    coords = torch.arange(size, dtype=torch.float)
    coords -= size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    g /= g.sum()
    return g.unsqueeze(0).unsqueeze(0)


def _make_desc(X, Y, taps, C1, C2, nonneg):
    """MMSsimDesc of (N,C,H,W) fp32 X and Y as they lie in memory (any strides); outputs and workspace left unset."""
    d = N.MMSsimDesc()
    d.N, d.C, d.H, d.W = X.shape
    d.x, d.y = X.data_ptr(), Y.data_ptr()
    d.x_strides[:] = list(X.stride())
    d.y_strides[:] = list(Y.stride())
    d.win_size = len(taps)
    d.win[:len(taps)] = taps
    d.C1, d.C2 = C1, C2
    d.flags = N.SSIM_NONNEG if nonneg else 0
    return d


class _SsimFn(torch.autograd.Function):
    """(X, Y) -> (reduced ssim, ssim per channel (N,C), cs per channel (N,C)); reduced = mean over (N,C) (``mean_c`` False) or over C."""

    @staticmethod
    def forward(ctx, X, Y, taps, C1, C2, nonneg, mean_c):
        dev = X.device
        Nn, C = X.shape[:2]
        d = _make_desc(X, Y, taps, C1, C2, nonneg)
        ssim_pc = torch.empty((Nn, C), device=dev, dtype=torch.float32)
        cs = torch.empty((Nn, C), device=dev, dtype=torch.float32)
        red = torch.empty((Nn,) if mean_c else (), device=dev, dtype=torch.float32)
        d.ssim, d.cs = ssim_pc.data_ptr(), cs.data_ptr()
        if mean_c:
            d.mean_c = red.data_ptr()
        else:
            d.mean_all = red.data_ptr()
        ws = N.workspace("mm_ssim_query_workspace", d, dev, at_least=1)       # (at least a byte: a zero-byte query must not pass NULL)
        N.call("mm_ssim_forward", dev, d)
        ctx.desc = d
        ctx.nonneg, ctx.mean_c = nonneg, mean_c
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(X, Y, ssim_pc)
        return red, ssim_pc, cs

    @staticmethod
    def backward(ctx, g_red, g_pc, g_cs):
        X, Y, ssim_pc = ctx.saved_tensors
        dev = X.device
        Nn, C = ssim_pc.shape
        g_s = None
        if g_red is not None:                        # d mean / d per-channel value, through the relu of nonnegative_ssim
            g_s = (g_red.reshape(Nn, 1) if ctx.mean_c else g_red.reshape(1, 1)) / (C if ctx.mean_c else Nn * C)
            g_s = g_s.expand(Nn, C)
            if ctx.nonneg:
                g_s = g_s * ~(ssim_pc <= 0)          # torch.relu's backward: cut where the value is <= 0, so a NaN plane passes
        if g_pc is not None:
            g_s = g_pc if g_s is None else g_s + g_pc
        if (g_s is None and g_cs is None) or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None, None, None, None
        g_s = None if g_s is None else g_s.to(dtype=torch.float32).contiguous()
        g_cs = None if g_cs is None else g_cs.to(dtype=torch.float32).contiguous()
        d = ctx.desc
        ws = N.workspace("mm_ssim_query_workspace", d, dev, at_least=1)
        gx = torch.empty(X.shape, device=dev, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        gy = torch.empty(Y.shape, device=dev, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        g = N.MMSsimGrads(N.ptr(g_s), N.ptr(g_cs), N.ptr(gx), N.ptr(gy))
        N.call("mm_ssim_backward", dev, d, g)
        return gx, gy, None, None, None, None, None


def _prepare(X, Y, win_size, win_sigma, win):
    """R7 + argument checks; returns (X, Y, taps as a list of fp32 values, win_size)."""
    if not X.shape == Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    for d in range(len(X.shape) - 1, 1, -1):
        X = X.squeeze(dim=d)
        Y = Y.squeeze(dim=d)
    if len(X.shape) == 5:
        raise NotImplementedError("volumetric (5-D) SSIM is not implemented on the MI355X path; pass (N,C,H,W) images")
    if len(X.shape) != 4:
        raise ValueError(f"Input images should be 4-d tensors, but got {X.shape}")
    if X.dtype != torch.float32 or Y.dtype != torch.float32:
        raise TypeError(f"the MI355X SSIM takes fp32 images, got {X.dtype} and {Y.dtype}")
    if win is not None:
        win_size = win.shape[-1]
    if not (win_size % 2 == 1):
        raise ValueError("Window size should be odd.")
    if win_size > N.SSIM_MAX_WIN:
        raise ValueError("win_size %d is above the largest the kernels take (%d)" % (win_size, N.SSIM_MAX_WIN))
    if win is None:
        return X, Y, _gauss_taps(win_size, win_sigma), win_size
    rows = win.detach().to("cpu", torch.float32).reshape(-1, win_size)
    if not bool((rows == rows[:1]).all()):
        raise ValueError("the window must be the same 1-D window for every channel")
    return X, Y, rows[0].tolist(), win_size


@functools.lru_cache(maxsize=16)
def _gauss_taps(size, sigma):
    """R1 as the list of fp32 values the descriptor takes (built once per (size, sigma): host time counts at the eval loop's sizes)"""
    return _fspecial_gauss_1d(size, sigma).reshape(-1).tolist()


def _on_device(X, Y):
    """(X, Y on one HIP device, device to return results on)"""
    if not X.is_cuda and not Y.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("ssim runs on the MI355X; no HIP device is available and there is no CPU fallback")
        return X.cuda(), Y.cuda(), X.device
    dev = X.device if X.is_cuda else Y.device
    return X.to(dev), Y.to(dev), dev


def _warn_skip(X, win_size):
    for i, s in enumerate(X.shape[2:]):
        if s < win_size:
            warnings.warn(f"Skipping Gaussian Smoothing at dimension 2+{i} for input: {X.shape} and win size: {win_size}")


def _constants(data_range, K):
    K1, K2 = K
    return float((K1 * data_range) ** 2), float((K2 * data_range) ** 2)


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03), nonnegative_ssim=False):
    """pytorch_msssim.ssim: SSIM of (N,C,H,W) fp32 images; a scalar (size_average) or (N,)."""
    X, Y, taps, win_size = _prepare(X, Y, win_size, win_sigma, win)
    Xd, Yd, out_dev = _on_device(X, Y)
    _warn_skip(Xd, win_size)
    C1, C2 = _constants(data_range, K)
    red, _, _ = _SsimFn.apply(Xd, Yd, taps, C1, C2, bool(nonnegative_ssim), not size_average)
    return red.to(out_dev)


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """pytorch_msssim.ms_ssim (R9), composed from the SSIM op's per-channel ssim and cs and F.avg_pool2d.  With device inputs nothing waits
    on the host, forward or backward: the weights go up from pinned memory, and the product over the levels is ``_prod_rows``."""
    X, Y, taps, win_size = _prepare(X, Y, win_size, win_sigma, win)
    smaller_side = min(X.shape[-2:])
    assert smaller_side > (win_size - 1) * (2 ** 4), \
        "Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % ((win_size - 1) * (2 ** 4))
    X, Y, out_dev = _on_device(X, Y)
    if weights is None:
        weights = MS_WEIGHTS
    weights_tensor = torch.as_tensor(weights, dtype=X.dtype).detach()
    if weights_tensor.is_cuda:
        weights_tensor = weights_tensor.to(X.device)
    else:                                                # through pinned memory, without waiting: new_tensor's copy from pageable memory blocks
        weights_tensor = weights_tensor.pin_memory().to(X.device, non_blocking=True)      # the host until the caller's stream has drained
    C1, C2 = _constants(data_range, K)
    levels = weights_tensor.shape[0]
    mcs = []
    for i in range(levels):
        _, ssim_per_channel, cs = _SsimFn.apply(X, Y, taps, C1, C2, False, False)
        if i < levels - 1:
            mcs.append(torch.relu(cs))
            padding = [s % 2 for s in X.shape[2:]]
            X = F.avg_pool2d(X, kernel_size=2, padding=padding)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=padding)
    ssim_per_channel = torch.relu(ssim_per_channel)
    mcs_and_ssim = torch.stack(mcs + [ssim_per_channel], dim=0)
    ms_ssim_val = _prod_rows(mcs_and_ssim ** weights_tensor.view(-1, 1, 1))
    return (ms_ssim_val.mean() if size_average else ms_ssim_val.mean(1)).to(out_dev)


def _prod_rows(t):
    """``torch.prod(t, dim=0)`` written out as multiplies, in the order its device kernel takes the rows in (four running products, row i into
    product i % 4, then the four combined in ascending order).  That the bits equal ``torch.prod``'s is measured on this stack (tests/test_gpu_ssim.py), not
    a contract: another torch build or another inner size may reduce in another order, and nothing here promises ``prod``'s bits.  Written out because ``prod``'s backward counts the zeros of
    its input on the host -- a wait for the caller's stream in every MS-SSIM backward; the chain's backward is plain multiplies, and a zero
    factor (a clamped level) needs no special case."""
    acc = [t[i] for i in range(min(4, t.shape[0]))]
    for i in range(4, t.shape[0]):
        acc[i % 4] = acc[i % 4] * t[i]
    out = acc[0]
    for a in acc[1:]:
        out = out * a
    return out


class SSIM(torch.nn.Module):
    """pytorch_msssim.SSIM"""

    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2, K=(0.01, 0.03),
                 nonnegative_ssim=False):
        super().__init__()
        if spatial_dims != 2:
            raise NotImplementedError("volumetric (spatial_dims=3) SSIM is not implemented on the MI355X path")
        self.win_size = win_size
        self.win = _fspecial_gauss_1d(win_size, win_sigma).repeat([channel, 1] + [1] * spatial_dims)
        self.size_average = size_average
        self.data_range = data_range
        self.K = K
        self.nonnegative_ssim = nonnegative_ssim

    def forward(self, X, Y):
        return ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win=self.win, K=self.K,
                    nonnegative_ssim=self.nonnegative_ssim)


class MS_SSIM(torch.nn.Module):
    """pytorch_msssim.MS_SSIM"""

    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2, weights=None,
                 K=(0.01, 0.03)):
        super().__init__()
        if spatial_dims != 2:
            raise NotImplementedError("volumetric (spatial_dims=3) MS-SSIM is not implemented on the MI355X path")
        self.win_size = win_size
        self.win = _fspecial_gauss_1d(win_size, win_sigma).repeat([channel, 1] + [1] * spatial_dims)
        self.size_average = size_average
        self.data_range = data_range
        self.weights = weights
        self.K = K

    def forward(self, X, Y):
        return ms_ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win=self.win, weights=self.weights, K=self.K)


def _mask_iou_rows(lhs, rhs):
    """sum(l*r) / (sum(l+r-l*r) + 1e-10) per image of two dense fp32 (B,H,W) device masks: the kernel of ``ops.mask_iou``"""
    B = lhs.shape[0]
    sums = torch.empty((B, 2), device=lhs.device, dtype=torch.float32)
    loss = torch.empty((), device=lhs.device, dtype=torch.float32)
    d = N.MMMaskIouDesc(B, lhs.numel() // B, N.ptr(lhs), N.ptr(rhs), N.ptr(sums), N.ptr(loss))
    N.call("mm_mask_iou_forward", lhs.device, d)
    return sums[:, 0] / (sums[:, 1] + 1e-10)


def recon_scores(pred, gt):
    """The reference's two evaluation numbers (trainer.py:771-795) for a whole batch: (B,4,H,W) fp32 pred and gt (RGB + mask) ->
    (ssim (B,), mask_iou (B,)): ``ssim`` over channels 0-2 with data_range=1, ``mask_iou`` = sum(l*r) / (sum(l+r-l*r) + 1e-10) over
    channel 3 (the same kernel as ``ops.mask_iou``; ``1 - mask_iou`` of one image is that function's value).

    The reference's loop scores images it has written to JPEG/PNG files and read back through a PIL resize; this helper scores the
    tensors themselves, so its values are not identical to the loop's.  ``recon_scores_as_saved`` scores what comes back from the files."""
    if pred.shape != gt.shape or pred.dim() != 4 or pred.shape[1] != 4:
        raise ValueError("recon_scores expects two (B,4,H,W) tensors, got %s / %s" % (tuple(pred.shape), tuple(gt.shape)))
    pred, gt, out_dev = _on_device(pred, gt)
    with torch.no_grad():
        s = ssim(pred[:, :3], gt[:, :3], data_range=1, size_average=False)
        iou = _mask_iou_rows(gt[:, 3].to(torch.float32).contiguous(), pred[:, 3].to(torch.float32).contiguous())
    return s.to(out_dev), iou.to(out_dev)


def recon_scores_as_saved(pred, gt, quality=100, white_gt=False, files=False):
    """``recon_scores`` as the reference's loop computes it: on the images it has SAVED as JPEG files and read back (trainer.py:697-795,
    test.py:302-455), all on the device.  (B,4,H,W) fp32 pred and gt -> (ssim (B,), mask_iou (B,)), the composition of
      1. ``export_images(x, "rgb+mask")``, rounding "trunc" (``to_pil_image``'s ``mul(255).byte()``); ``white=white_gt`` for gt only (the
         ``opt.bg`` branch, trainer.py:754-757);
      2. ``jpeg_roundtrip`` of the rgb in mode "RGB" (a 4:2:0 colour file, ``.convert('RGB')``) and of the mask in mode "L" (a greyscale
         file, ``.convert('L')``), ``as_float``: ``to_tensor`` of the reopened images;
      3. ``ssim(ori, rec, data_range=1, size_average=False)`` and the mask-IoU kernel of ``recon_scores``.
    The ``.resize`` between open and score asks for the file's own size, which is the identity.  Equal, with torch.equal, to that
    composition written out from the public functions.

    files=True: ``(ssim, mask_iou, (ori, ori_mask, rec, rec_mask))``, the third being the four ``JpegBatch``es the loop writes, B files
    each: the colour ones from the round trip's own transform pass (``jpeg_roundtrip(files=True)``), the two masks from
    ``encode_jpeg(mask, quality, mode="L")``.  The masks' transform therefore runs twice, once inside the round trip (which keeps a block in
    registers and forms no file) and once for the file: a mask is a third of a frame's bytes and one block an MCU, so the second pass
    costs less than the copy it saves.  The scores are torch.equal to those of files=False."""
    from .export import export_images
    from .jpeg import encode_jpeg, jpeg_roundtrip
    if pred.shape != gt.shape or pred.dim() != 4 or pred.shape[1] != 4:
        raise ValueError("recon_scores_as_saved expects two (B,4,H,W) tensors, got %s / %s" % (tuple(pred.shape), tuple(gt.shape)))
    pred, gt, out_dev = _on_device(pred, gt)
    with torch.no_grad():
        back, saved = [], []
        for x, white in ((gt, bool(white_gt)), (pred, False)):
            rgb, mask = export_images(x, "rgb+mask", rounding="trunc", white=white)
            colour = jpeg_roundtrip(rgb, quality, "RGB", as_float=True, files=bool(files))
            if files:
                colour, batch = colour
                saved += [batch, encode_jpeg(mask, quality, mode="L")]
            back.append((colour, jpeg_roundtrip(mask, quality, "L", as_float=True)))
        (ori, ori_mask), (rec, rec_mask) = back
        s = ssim(ori, rec, data_range=1, size_average=False)
        iou = _mask_iou_rows(ori_mask, rec_mask)
    return (s.to(out_dev), iou.to(out_dev)) + ((tuple(saved),) if files else ())
