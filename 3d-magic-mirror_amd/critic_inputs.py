"""Critic inputs of the GAN step: host side of ``mm_critic_inputs_forward / _backward`` (csrc/mm_critic.hip).

``critic_inputs(Xa, Xer90, Xir, unmask)`` replaces what the reference's trainer.py:370-411 and :429-431 build around its discriminator
-- three compositions over white, three ``detach().clone()`` copies, two ``cat`` and the two gradient-penalty interpolates with their
host-drawn alphas -- by one launch forward and one backward.  The renders' NHWC memory is read as it is and the batches come out
NCHW-contiguous; the gradient goes back to each fake in that fake's own layout, so a render's gradient reaches its node without a copy.

With ``M`` the channel map of the ``unmask`` mode (``m = X[:, 3:4]``)

    unmask 0 (C = 3)   M(X) = X[:, :3] * m + (1 - m)        the image over white with its own alpha (smr_utils.py:198-202)
    unmask 1 (C = 3)   M(X) = X[:, :3]
    unmask 2 (C = 4)   M(X) = X

every forward value is torch's eager fp32 result bit for bit.  Device tensors only."""
import collections

import torch

from . import _native as N
from .interpolate import _alpha

CriticInputs = collections.namedtuple("CriticInputs", ("d_batch", "g_batch", "gp_er90", "gp_ir", "alphas"))
CriticInputs.__doc__ = """What ``critic_inputs`` returns.

d_batch (3B,C,H,W): cat(M(Xa), M(Xer90), M(Xir)), requires_grad False -- the D step's batch (trainer.py:391/393).
g_batch (2B,C,H,W): cat(M(Xer90), M(Xir)), differentiable w.r.t. Xer90 and Xir -- the G step's batch (trainer.py:429/431).  It IS rows
    [B, 3B) of d_batch's memory: neither tensor may be written in place.
gp_er90, gp_ir (B,C,H,W): a1 * M(Xa) + ((1 - a1) * M(Xer90)) and a2 * M(Xa) + ((1 - a2) * M(Xir)) as fresh leaves with requires_grad
    True (smr_utils.py:340-346), or None with ``gp=False``.
alphas: the two (B,) alphas used, or None with ``gp=False``."""


def _layout(x):
    """(tensor the kernel reads, its layout flag): NCHW-contiguous (0) and NHWC-dense (1) are read in place, anything else is copied"""
    if x.is_contiguous():
        return x, 0
    if x.permute(0, 2, 3, 1).is_contiguous():
        return x, 1
    return x.contiguous(), 0


def _desc(B, H, W, unmask, xs, flags):
    d = N.MMCriticDesc()
    d.B, d.H, d.W, d.unmask = B, H, W, unmask
    d.Xa, d.Xer90, d.Xir = (N.ptr(x) for x in xs)
    d.Xa_nhwc, d.Xer90_nhwc, d.Xir_nhwc = flags
    return d


class _CriticFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Xa, Xer90, Xir, a1, a2, unmask):
        ctx.set_materialize_grads(False)
        B, _, H, W = Xa.shape
        C = 4 if unmask == 2 else 3
        flags = tuple(1 if not x.is_contiguous() else 0 for x in (Xa, Xer90, Xir))      # (critic_inputs passes one of the two layouts)
        buf = torch.empty((3 * B, C, H, W), dtype=torch.float32, device=Xa.device)
        gp1 = gp2 = None
        d = _desc(B, H, W, unmask, (Xa, Xer90, Xir), flags)
        if a1 is not None:
            gp1, gp2 = torch.empty((B, C, H, W), dtype=torch.float32, device=Xa.device), torch.empty((B, C, H, W), dtype=torch.float32, device=Xa.device)
            d.alpha_er90, d.alpha_ir, d.out_gp_er90, d.out_gp_ir = N.ptr(a1), N.ptr(a2), N.ptr(gp1), N.ptr(gp2)
        d.out_batch = N.ptr(buf)
        N.call("mm_critic_inputs_forward", Xa.device, d)
        ctx.unmask, ctx.flags = unmask, flags
        ctx.save_for_backward(*((Xer90, Xir) if unmask == 0 else ()))            # d m reads the fakes; the other modes read nothing
        ctx.meta = tuple((tuple(x.shape), tuple(x.stride())) for x in (Xer90, Xir))
        g = buf.narrow(0, B, 2 * B)                                              # the G step's batch: the same memory, differentiable
        nd = [buf] + [t for t in (gp1, gp2) if t is not None]
        ctx.mark_non_differentiable(*nd)
        return buf, g, gp1, gp2

    @staticmethod
    def backward(ctx, _g_buf, g, _g1, _g2):
        need = ctx.needs_input_grad[1:3]
        if g is None or not any(need):
            return (None,) * 6
        g = g.to(torch.float32).contiguous()
        (shape, _), _ = ctx.meta
        B, _, H, W = shape
        xs = ctx.saved_tensors if ctx.unmask == 0 else (None, None)
        d = _desc(B, H, W, ctx.unmask, (None,) + tuple(xs), ctx.flags)
        grads = [torch.empty_strided(sh, st, dtype=torch.float32, device=g.device) if n else None for (sh, st), n in zip(ctx.meta, need)]
        gr = N.MMCriticGrads()
        gr.g_batch, gr.grad_er90, gr.grad_ir = N.ptr(g), N.ptr(grads[0]), N.ptr(grads[1])
        gr.grad_er90_nhwc, gr.grad_ir_nhwc = ctx.flags[1], ctx.flags[2]
        N.call("mm_critic_inputs_backward", g.device, d, gr)
        return None, grads[0], grads[1], None, None, None


def critic_inputs(Xa, Xer90, Xir, unmask=0, gp_alphas=None, gp=True, generator=None):
    """The discriminator's image batches of one GAN iteration (trainer.py:370-411, 429-431) as a ``CriticInputs``.

    Xa (the real images), Xer90 and Xir (the two fakes): float (B,4,H,W) tensors on one device.  NCHW-contiguous and NHWC-dense
    (strides (4HW, 1, 4W, 4): what ``DiffRender.render`` returns) are read in place, the layout chosen per input; any other strides go
    through ``.contiguous()``, other float dtypes through ``.float()``.  Xa never receives a gradient.  Xer90 and Xir may be the same
    tensor (``--hard`` off, or ``lambda_ic == 0``): autograd then sums the two gradients.  Each fake's gradient has that fake's strides.

    unmask: the reference's ``--unmask`` mode, 0, 1 or 2 (the module docstring has the three channel maps).
    gp_alphas: a pair of float32 (B,) or (B,1,1,1) device tensors that do not require grad, the weights of the real image in the two
    gradient-penalty interpolates.  None: drawn on the device by ``torch.rand`` (from ``generator`` when given), one (2,B) draw with
    no host draw and no upload.  The distribution is the reference's U[0,1); the random stream is NOT (the reference draws them with
    numpy on the host).  gp=False skips both interpolates: no buffers are made, ``gp_er90``, ``gp_ir`` and ``alphas`` are None.

    ``g_batch`` is rows [B, 3B) of ``d_batch``'s memory (the reference computes the same values twice): neither may be written in
    place.  The backward is one launch without atomics, bitwise reproducible: for unmask 0 ``d rgb_c = g_c * m`` and
    ``d m = sum_c g_c * (rgb_c - 1)`` summed in ascending c; for unmask 1 ``d rgb = g`` and ``d m = 0``; for unmask 2 the identity."""
    xs = (Xa, Xer90, Xir)
    names = ("Xa", "Xer90", "Xir")
    for x, nm in zip(xs, names):
        if not torch.is_tensor(x) or not x.dtype.is_floating_point:
            raise ValueError("%s must be a float tensor, got %s" % (nm, x.dtype if torch.is_tensor(x) else type(x)))
        if x.dim() != 4 or x.shape[1] != 4 or min(x.shape) < 1:
            raise ValueError("%s must have shape (B,4,H,W), got %s" % (nm, tuple(x.shape)))
        if tuple(x.shape) != tuple(Xa.shape):
            raise ValueError("%s has shape %s, Xa %s" % (nm, tuple(x.shape), tuple(Xa.shape)))
        if x.device != Xa.device:
            raise ValueError("%s is on %s, Xa on %s" % (nm, x.device, Xa.device))
    if unmask not in (0, 1, 2):
        raise ValueError("unmask must be 0, 1 or 2, got %r" % (unmask,))
    B, dev = Xa.shape[0], Xa.device
    a1 = a2 = None
    if gp and gp_alphas is not None:
        if len(gp_alphas) != 2:
            raise ValueError("gp_alphas must be a pair of tensors")
        a1, a2 = _alpha(gp_alphas[0], B, dev, "gp_alphas[0]"), _alpha(gp_alphas[1], B, dev, "gp_alphas[1]")
    N.require_device(*xs)
    if gp and gp_alphas is None:
        r = torch.rand((2, B), dtype=torch.float32, device=dev, generator=generator)
        a1, a2 = r[0], r[1]
    same = Xir is Xer90
    Xa = _layout(Xa.detach() if Xa.dtype == torch.float32 else Xa.detach().float())[0]
    Xer90 = _layout(Xer90 if Xer90.dtype == torch.float32 else Xer90.float())[0]
    Xir = Xer90 if same else _layout(Xir if Xir.dtype == torch.float32 else Xir.float())[0]
    buf, g, gp1, gp2 = _CriticFn.apply(Xa, Xer90, Xir, a1, a2, int(unmask))
    if gp1 is not None:
        gp1.requires_grad_(True)
        gp2.requires_grad_(True)
    return CriticInputs(buf, g, gp1, gp2, None if a1 is None else (a1, a2))
