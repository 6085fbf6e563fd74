"""Disentangle regularisation of the generator step (``--dis1`` / ``--dis2``, trainer.py:455-494): host side of ``mm_disentangle_inputs``
and ``mm_disentangle_forward / _backward`` (csrc/mm_disentangle.hip).

    draw_erase_box        the box ``torchvision.transforms.RandomErasing`` would draw, on the host, from torch's CPU generator
    disentangle_inputs    ``fliplr(Xa)`` and ``RandomErasing(p=1)(Xa)``, the two extra encoder batches, in one launch
    disentangle_terms     the seven means of the block as a (7,) tensor, one launch forward and one backward, gradients to BOTH sets

``DiffRender.recon_disentangle`` composes the reference's scalar from the terms.  Device tensors only (``draw_erase_box`` apart)."""
import math

import torch

from . import _native as N
from .critic_inputs import _layout

TEXT, SHAPE_FLIP, AZIM, ELEV, DIST, BIAS, SHAPE_JITTER = range(7)
BASE_KEYS = ("textures", "vertices", "azimuths", "elevations", "distances", "biases", "delta_vertices")
FLIP_KEYS = ("textures", "vertices")
JITTER_KEYS = ("azimuths", "elevations", "distances", "biases", "delta_vertices")


def draw_erase_box(hw, scale=(0.02, 0.33), ratio=(0.3, 3.3), p=1.0, generator=None):
    """The box ``RandomErasing(p, scale, ratio)`` erases in an image of ``hw = (H, W)``: ``(i, j, h, w)`` -- rows [i, i+h), columns
    [j, j+w) -- or None when nothing is erased (``p`` fails, or ten attempts find no box smaller than the image).

    ``RandomErasing.forward`` + ``get_params`` restated on torch's CPU generator (``generator``, or the global one), the same calls in the
    same order, so that a seeded run draws what the reference draws: ``torch.rand(1) < p``; then up to ten times
    ``area * torch.empty(1).uniform_(scale[0], scale[1]).item()``, ``exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()`` with
    ``log_ratio = torch.log(torch.tensor(ratio))``, ``h = int(round(sqrt(area * aspect)))``, ``w = int(round(sqrt(area / aspect)))``, next
    attempt unless ``h < H and w < W``, else ``torch.randint(0, H - h + 1, (1,))`` and ``torch.randint(0, W - w + 1, (1,))``.
    [recall-risk: torchvision is not installed where this was written; the call sequence is restated from memory.  With ``value=0``, the
    reference's, ``get_params`` draws nothing for the fill.]"""
    H, W = int(hw[0]), int(hw[1])
    if not (torch.rand(1, generator=generator) < p):
        return None
    area = H * W
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        erase_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator)).item()
        h = int(round(math.sqrt(erase_area * aspect_ratio)))
        w = int(round(math.sqrt(erase_area / aspect_ratio)))
        if not (h < H and w < W):
            continue
        i = torch.randint(0, H - h + 1, size=(1,), generator=generator).item()
        j = torch.randint(0, W - w + 1, size=(1,), generator=generator).item()
        return i, j, h, w
    return None


def disentangle_inputs(Xa, box, value=0.0, flip=True, erase=True):
    """``(X_flip, X_erase)``: ``fliplr(Xa)`` (trainer.py:462) and ``RandomErasing(p=1)(Xa)`` (:476-479), both made by ONE launch that reads
    every element of ``Xa`` once; either is None when not asked for (``flip`` / ``erase``).  Pure copies: bit for bit torch's.

    Xa: float32 (B,C,H,W) on the device.  NCHW-contiguous (the loader's batch) and NHWC-dense (a render) are read in place, anything else
    goes through ``.contiguous()``.  Both outputs are NCHW-contiguous, separate tensors (the encoders have BatchNorm and the reference calls
    ``netE`` once per batch), and carry no gradient: ``Xa`` is data.
    X_flip[b,c,y,x] = Xa[b,c,y,W-1-x].
    X_erase: ``Xa`` with ``value`` in ALL C channels of rows [i, i+h), columns [j, j+w) -- the mask channel too, as the reference's
    ``value=0`` does.  ``box``: None erases nothing (a copy); a 4-tuple ``(i, j, h, w)`` is the reference's form, one box for the whole
    batch (``draw_erase_box``), passed as kernel arguments; an int32 (B,4) device tensor gives one box per sample, read by the kernel without
    a synchronisation.  Boxes are clamped to the image on the device; ``h`` or ``w`` below 1 erases nothing."""
    if not torch.is_tensor(Xa) or Xa.dtype != torch.float32 or Xa.dim() != 4 or min(Xa.shape) < 1:
        raise ValueError("Xa must be a float32 (B,C,H,W) tensor, got %s" % (tuple(Xa.shape) if torch.is_tensor(Xa) else type(Xa),))
    N.require_device(Xa)
    if not flip and not erase:
        return None, None
    B, C, H, W = Xa.shape
    x, nhwc = _layout(Xa.detach())
    d = N.MMDisentangleInputsDesc()
    d.B, d.C, d.H, d.W, d.nhwc, d.value = B, C, H, W, nhwc, float(value)
    keep = None
    if torch.is_tensor(box):
        if box.dtype != torch.int32 or tuple(box.shape) != (B, 4) or box.device != Xa.device:
            raise ValueError("a box tensor must be int32 (B,4) on Xa's device, got %s %s on %s" % (box.dtype, tuple(box.shape), box.device))
        keep = box.contiguous()
        d.boxes, d.boxes_rows = N.ptr(keep), B
    elif box is not None:
        if len(box) != 4:
            raise ValueError("box must be None, (i, j, h, w) or an int32 (B,4) tensor")
        d.box[0], d.box[1], d.box[2], d.box[3] = (int(v) for v in box)
    out_flip = torch.empty((B, C, H, W), dtype=torch.float32, device=Xa.device) if flip else None
    out_erase = torch.empty((B, C, H, W), dtype=torch.float32, device=Xa.device) if erase else None
    d.x, d.out_flip, d.out_erase = N.ptr(x), N.ptr(out_flip), N.ptr(out_erase)
    N.call("mm_disentangle_inputs", Xa.device, d)
    return out_flip, out_erase


def _desc(B, V, Ht, Wt, ts):
    d = N.MMDisentangleDesc()
    d.B, d.V, d.Ht, d.Wt = B, V, Ht, Wt
    for k, t in zip(N.DISENTANGLE_TENSORS, ts):
        setattr(d, k, N.ptr(t))
    return d


class DisentangleFn(torch.autograd.Function):
    """terms (7,) = [l_text, l_shape_flip, l_azim, l_elev, l_dist, l_bias, l_shape_jitter]; inputs: (B, V, Ht, Wt), then the fourteen tensors of
    ``_native.DISENTANGLE_TENSORS`` -- seven of Ae, two of Ae_fliplr (both or None), five of Ae_jitter (all or None)."""

    @staticmethod
    def forward(ctx, cfg, *tensors):
        given = [t for t in tensors if t is not None]
        N.require_device(*given)
        dev = given[0].device
        ts = [None if t is None else t.detach().to(device=dev, dtype=torch.float32).contiguous() for t in tensors]
        B, V, Ht, Wt = cfg
        shapes = {"textures": (B, 3, Ht, Wt), "vertices": (B, V, 3), "azimuths": (B,), "elevations": (B,), "distances": (B,), "biases": (B, 2),
                  "delta_vertices": (B, V, 3)}
        for k, t in zip(N.DISENTANGLE_TENSORS, ts):
            want = shapes[k.split("_", 1)[1] if k.startswith(("flip_", "jitter_")) else k]
            if t is not None and (t.numel() != math.prod(want) or (len(want) > 1 and tuple(t.shape) != want)):
                raise RuntimeError("disentangle_terms: %s must be %s, got %s" % (k, want, tuple(t.shape)))
        terms = torch.empty(7, device=dev, dtype=torch.float32)
        d = _desc(B, V, Ht, Wt, ts)
        d.terms = N.ptr(terms)
        ws = N.workspace("mm_disentangle_query_workspace", d, dev, zero=True)     # zero-filled: ABI contract
        N.call("mm_disentangle_forward", dev, d)
        ctx.cfg = cfg
        ctx.present = [t is not None for t in ts]
        ctx.meta = [None if t is None else (t.shape, t.dtype) for t in tensors]
        ctx.save_for_backward(*[t for t in ts if t is not None], ws)
        return terms

    @staticmethod
    def backward(ctx, g):
        *saved, ws = ctx.saved_tensors
        it = iter(saved)
        ts = [next(it) if p else None for p in ctx.present]
        need = [n and p for n, p in zip(ctx.needs_input_grad[1:], ctx.present)]
        if not any(need):
            return (None,) * 15
        dev = ws.device
        d = _desc(*ctx.cfg, ts)
        d.workspace, d.workspace_bytes = N.ptr(ws), ws.numel()                    # the forward's: it holds the per-sample norms
        grads = [torch.empty_like(t) if n else None for t, n in zip(ts, need)]
        w = g.detach().to(device=dev, dtype=torch.float32).contiguous()
        gr = N.MMDisentangleGrads()
        gr.weights = N.ptr(w)
        for k, t in zip(N.DISENTANGLE_TENSORS, grads):
            setattr(gr, k, N.ptr(t))
        N.call("mm_disentangle_backward", dev, d, gr)
        return (None,) + tuple(None if t is None else t.reshape(m[0]).to(m[1]) for t, m in zip(grads, ctx.meta))


def disentangle_terms(Ae, Ae_fliplr=None, Ae_jitter=None):
    """The seven terms of the disentangle block as a float32 (7,) tensor, differentiable w.r.t. every attribute it reads in all three sets
    (the reference detaches none):

      [0] l_text          mean over B*3*Ht*Wt of |Tf[b,c,y,Wt-1-x] - T[b,c,y,x]|                    (Tf = Ae_fliplr's textures, read mirrored)
      [1] l_shape_flip    mean over b of sqrt(sum_{v,k} (Vf[b,v,k] - s_k V[b,v,k])^2), s = (-1, 1, 1)   (vertices)
      [2] l_azim, [3] l_elev   mean over B*2 of the squared differences of (cos, sin) of the angle in degrees (angle2xy)
      [4] l_dist (mean over B), [5] l_bias (mean over B*2) of squared differences
      [6] l_shape_jitter  mean over b of sqrt(sum (dVj[b] - dV[b])^2)                                (delta_vertices)

    Terms 0-1 need ``Ae_fliplr``, terms 2-6 ``Ae_jitter``; a missing set leaves its terms 0 and nothing of it, or of the attributes of ``Ae``
    only it is compared with, is read.  Half and double inputs are converted to fp32 on the host.  The sums are added in a fixed order
    without float atomics: the same bits run to run.  A norm term's gradient is exactly 0 for a sample whose difference is all zero, and a
    texel whose difference is exactly 0 gets 0 -- torch's rules."""
    if Ae_fliplr is None and Ae_jitter is None:
        raise ValueError("disentangle_terms needs Ae_fliplr, Ae_jitter or both")
    flat = lambda A, k: A[k].reshape(-1) if k in ("azimuths", "elevations", "distances") else A[k]
    base = [flat(Ae, k) if ((Ae_fliplr is not None and k in FLIP_KEYS) or (Ae_jitter is not None and k in JITTER_KEYS)) else None for k in BASE_KEYS]
    f = [None if Ae_fliplr is None else Ae_fliplr[k] for k in FLIP_KEYS]
    j = [None if Ae_jitter is None else flat(Ae_jitter, k) for k in JITTER_KEYS]
    B, V = Ae["vertices"].shape[:2]
    Ht, Wt = Ae["textures"].shape[2:]
    return DisentangleFn.apply((int(B), int(V), int(Ht), int(Wt)), *base, *f, *j)
