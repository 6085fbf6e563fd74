"""Attribute interpolation of the generator step: host side of ``mm_collapse_resample / mm_attribute_mix_*`` (csrc/mm_interp.hip).

``interpolate_attributes(Ae, opt, elev_range, dist_range)`` replaces the reference's trainer.py:279-342 -- the hard view ``Ae90`` and
the interpolated attribute set ``Ai`` built between render #1 and render #2 -- without a device-to-host copy: the collapse test and
the resampling of the two permutations run on the device (``resample_collapsed``), and the nine gathers, clones and five lerps are
one launch each way (``mix_attributes``).

``mix_attributes`` computes ``X = a * A[X][idx_a] + (1 - a) * A[X][idx_b]`` bit for bit as torch's eager fp32 composition does; its
backward sums every source row's terms in a fixed order, atomic-free and bitwise reproducible (for permutations of fp32 sources it
equals torch autograd bit for bit).  Device tensors only."""
import random

import numpy as np
import torch

from . import _native as N

MIX_KEYS = ("vertices", "delta_vertices", "textures", "bg", "lights")
COPY_KEYS = ("azimuths", "bg", "biases", "elevations", "distances", "vertices", "delta_vertices", "textures", "lights")  # deep_copy's
_FLOATS = (torch.float32, torch.float16, torch.bfloat16)


# ---- validation: every shape is checked here, before anything reaches a kernel -------------------------------------------------
def _indices(idx, B, dev, name):
    """``idx`` as a (B,) int32 tensor on ``dev``, with no synchronisation.  Host indices (numpy, lists, CPU tensors) are checked for
    length and range here and uploaded from pinned memory; device indices are checked for length only -- a value outside [0, B)
    becomes -1, and the kernel writes that output row as NaN."""
    if torch.is_tensor(idx) and idx.device.type != "cpu":
        if idx.device != dev:
            raise ValueError("%s is on %s, the attributes on %s" % (name, idx.device, dev))
        if idx.dim() != 1 or idx.shape[0] != B or idx.dtype.is_floating_point or idx.dtype.is_complex or idx.dtype == torch.bool:
            raise ValueError("%s must be a (%d,) integer tensor, got %s %s" % (name, B, tuple(idx.shape), idx.dtype))
        i = idx.detach()
        if i.dtype != torch.int32:                       # narrowing must not wrap a large value into range
            i = i.masked_fill((i < 0) | (i >= B), -1).to(torch.int32)
        return i.contiguous()
    a = idx.detach().numpy() if torch.is_tensor(idx) else np.asarray(idx)
    if a.ndim != 1 or a.shape[0] != B or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s must hold %d integers, got shape %s dtype %s" % (name, B, a.shape, a.dtype))
    if a.min() < 0 or a.max() >= B:
        raise ValueError("%s holds indices outside [0, %d): min %d, max %d" % (name, B, int(a.min()), int(a.max())))
    return N.upload_int32(a, dev)[1]


def _alpha(a, B, dev, name):
    if not torch.is_tensor(a):
        raise ValueError("%s must be a tensor" % name)
    if a.requires_grad:
        raise RuntimeError("%s is a constant of the interpolation (the reference draws it), but it requires grad" % name)
    if a.dim() < 1 or a.shape[0] != B or a.numel() != B:
        raise ValueError("%s must have shape (%d,) or (%d,1,...), got %s" % (name, B, B, tuple(a.shape)))
    if a.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (name, a.dtype))
    if a.device != dev:
        raise ValueError("%s is on %s, the attributes on %s" % (name, a.device, dev))
    return a.reshape(B).contiguous()


def _source(A, key, shape, dev):
    t = A[key]
    if not torch.is_tensor(t) or t.dtype not in _FLOATS:
        raise ValueError("A[%r] must be a float32, float16 or bfloat16 tensor, got %s" % (key, t.dtype if torch.is_tensor(t) else type(t)))
    if tuple(t.shape) != shape:
        raise ValueError("A[%r] must have shape %s, got %s" % (key, shape, tuple(t.shape)))
    if t.device != dev:
        raise ValueError("A[%r] is on %s, A['vertices'] on %s" % (key, t.device, dev))
    return (t if t.dtype == torch.float32 else t.float()).contiguous()   # torch's type promotion gives fp32 outputs anyway


# ---- the mix ----------------------------------------------------------------------------------------------------------------------
def _desc(shapes, ia, ib, alphas):
    """the descriptor's sizes, indices and alphas; shapes: the five sources' shapes (bg's None when absent)"""
    v, _, tex, bg, _ = shapes
    d = N.MMInterpDesc()
    d.B, d.V = v[0], v[1]
    d.Ht, d.Wt = tex[2], tex[3]
    if bg is not None:
        d.H, d.W = bg[2], bg[3]
    d.idx_a, d.idx_b = N.ptr(ia), N.ptr(ib)
    d.alpha_shape, d.alpha_texture, d.alpha_light = (N.ptr(a) for a in alphas)
    return d


class _MixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ia, ib, a_shape, a_texture, a_light, vertices, delta_vertices, textures, bg, lights):
        ctx.set_materialize_grads(False)
        srcs = (vertices, delta_vertices, textures, bg, lights)
        outs = tuple(None if t is None else torch.empty_like(t) for t in srcs)
        alphas = (a_shape, a_texture, a_light)
        ctx.shapes = tuple(None if t is None else tuple(t.shape) for t in srcs)
        d = _desc(ctx.shapes, ia, ib, alphas)
        d.vertices, d.delta_vertices, d.textures, d.bg, d.lights = (N.ptr(t) for t in srcs)
        d.out_vertices, d.out_delta_vertices, d.out_textures, d.out_bg, d.out_lights = (N.ptr(t) for t in outs)
        N.call("mm_attribute_mix_forward", vertices.device, d)
        ctx.save_for_backward(ia, ib, *alphas)                  # the backward needs the sources' shapes only, not their data
        ctx.has_bg = bg is not None
        return tuple(o for o in outs if o is not None)

    @staticmethod
    def backward(ctx, *gs):
        ia, ib, a_shape, a_texture, a_light = ctx.saved_tensors
        gs = list(gs)
        if not ctx.has_bg:
            gs.insert(3, None)
        need = ctx.needs_input_grad[5:]
        ups, dst = [None] * 5, [None] * 5
        for k in range(5):
            if gs[k] is not None and need[k]:
                ups[k] = gs[k].to(torch.float32).contiguous()
                dst[k] = torch.empty(ctx.shapes[k], dtype=torch.float32, device=ia.device)
        if all(u is None for u in ups):
            return (None,) * 10
        d = _desc(ctx.shapes, ia, ib, (a_shape, a_texture, a_light))
        ws = N.workspace("mm_interp_query_workspace", d, ia.device)
        gr = N.MMInterpGrads(*[N.ptr(t) for t in ups + dst])
        N.call("mm_attribute_mix_backward", ia.device, d, gr)
        return (None,) * 5 + tuple(dst)


def mix_attributes(A, idx_a, idx_b, alpha_shape, alpha_texture, alpha_light):
    """{vertices, delta_vertices, textures, bg, lights} with ``X = alpha * A[X][idx_a] + (1 - alpha) * A[X][idx_b]``: trainer.py:331-340
    applied to ``deep_copy(A, idx_a)`` and ``deep_copy(A, idx_b)``, one launch.  alpha_shape weighs vertices and delta_vertices,
    alpha_texture textures and bg, alpha_light lights.

    A: vertices (B,V,3), delta_vertices (B,V,3), textures (B,3,Ht,Wt), bg (B,3,H,W) or None / absent, lights (B,9); fp32, fp16 or
    bf16, any strides, in device memory (fp16 / bf16 are upcast: the outputs are fp32, as torch's type promotion makes them).
    idx_a, idx_b: (B) integer indices; on the host (numpy, list or CPU tensor) they are range-checked here, on the device a value
    outside [0, B) gives a NaN output row.  Alphas: float32 constants of shape (B) or the reference's (B,1,...) shapes."""
    v = A["vertices"]
    present = [A[k] for k in MIX_KEYS if A.get(k) is not None]
    if not all(torch.is_tensor(t) for t in present):
        raise ValueError("mix_attributes expects tensors in A")
    N.require_device(*present)
    if v.dim() != 3 or v.shape[2] != 3 or min(v.shape) < 1:
        raise ValueError("A['vertices'] must have shape (B,V,3), got %s" % (tuple(v.shape),))
    B, V, dev = v.shape[0], v.shape[1], v.device
    tex, bg = A["textures"], A.get("bg")
    if not torch.is_tensor(tex) or tex.dim() != 4:
        raise ValueError("A['textures'] must have shape (B,3,Ht,Wt)")
    if bg is not None and (not torch.is_tensor(bg) or bg.dim() != 4):
        raise ValueError("A['bg'] must have shape (B,3,H,W) or be None")
    srcs = (_source(A, "vertices", (B, V, 3), dev), _source(A, "delta_vertices", (B, V, 3), dev),
            _source(A, "textures", (B, 3) + tuple(tex.shape[2:]), dev),
            None if bg is None else _source(A, "bg", (B, 3) + tuple(bg.shape[2:]), dev), _source(A, "lights", (B, 9), dev))
    alphas = (_alpha(alpha_shape, B, dev, "alpha_shape"), _alpha(alpha_texture, B, dev, "alpha_texture"),
              _alpha(alpha_light, B, dev, "alpha_light"))
    ia, ib = _indices(idx_a, B, dev, "idx_a"), _indices(idx_b, B, dev, "idx_b")
    outs = list(_MixFn.apply(ia, ib, *alphas, *srcs))
    if bg is None:
        outs.insert(3, None)
    return dict(zip(MIX_KEYS, outs))


# ---- collapse resampling ----------------------------------------------------------------------------------------------------------
def resample_collapsed(delta_vertices, idx_a, idx_b, uniforms, threshold=0.4):
    """(idx_a, idx_b, n_bad) as new device tensors (int32 (B), int32 (B), int32 ()), with no synchronisation: trainer.py:293-306
    (opt.inv == 0).  Sample b is bad when mean(|delta_vertices[b, -1, :]|) = ((|x| + |y|) + |z|) / 3 > threshold in fp32 (a NaN mean
    is not bad).  Every slot of idx_a that holds a bad sample gets good[min(floor(uniforms[0, s] * n_good), n_good - 1)], good being
    the samples that are not bad in ascending order; idx_b likewise with uniforms[1].  The result has the distribution of the
    reference's ``np.random.choice(good)`` draws, not its random stream.  Where the reference raises (no good sample), the indices
    come back unchanged and n_bad == B.  uniforms: (2,B) float32 in [0, 1) on the device."""
    N.require_device(delta_vertices)
    dv = delta_vertices
    if dv.dim() != 3 or dv.shape[2] != 3 or dv.shape[0] < 1 or dv.shape[1] < 1 or dv.dtype not in _FLOATS:
        raise ValueError("delta_vertices must be a (B,V,3) float tensor, got %s %s" % (tuple(dv.shape), dv.dtype))
    B, dev = dv.shape[0], dv.device
    dv = dv.detach()
    if dv.dtype != torch.float32 or not dv.is_contiguous():
        dv = dv[:, -1:, :].float().contiguous()               # only the last vertex is read
    if not torch.is_tensor(uniforms) or tuple(uniforms.shape) != (2, B) or uniforms.dtype != torch.float32 or uniforms.device != dev:
        raise ValueError("uniforms must be a (2,%d) float32 tensor on %s" % (B, dev))
    u = uniforms.detach().contiguous()
    ia = _indices(idx_a, B, dev, "idx_a").clone()
    ib = _indices(idx_b, B, dev, "idx_b").clone()
    n_bad = torch.empty((), dtype=torch.int32, device=dev)
    N.call("mm_collapse_resample", dev, B, dv.shape[1], N.ptr(dv), N.ptr(ia), N.ptr(ib), N.ptr(u), float(threshold), N.ptr(n_bad))
    return ia, ib, n_bad


# ---- the whole block --------------------------------------------------------------------------------------------------------------
def interpolate_attributes(Ae, opt, elev_range, dist_range, generator=None):
    """(Ai, Ae90) of trainer.py:279-342, up to the render, with no device-to-host copy.

    Ae: the attributes after render #1; opt: the reference's options (hard, hard_range, inv, lambda_ic, azi_scope, bias_range, beta,
    bg); elev_range / dist_range: (netE.camera_enc.elev_min, elev_max) and (dist_min, dist_max) as floats.

    Draws what the reference draws, in its order, from the same generators: Python ``random`` and the global CUDA generator for the
    hard view, numpy for the two permutations, the global CUDA generator for the interpolation (the unused alpha_camera included).
    The resampling uniforms (2,B) come last, from ``generator`` (default: the global CUDA generator), and only when resampling runs
    (opt.inv == 0 and opt.lambda_ic > 0): every value the reference draws here is reproduced, and later draws on that generator
    are shifted by 2B.  The reference's ``np.random.choice`` draws are not made, so numpy's stream differs from the reference's
    after an iteration with a collapsed sample; a caller who needs that stream computes the indices on the host and calls
    ``mix_attributes``.

    Ae90 (opt.hard, else None) holds Ae's deep_copy keys as the same tensors (render only reads them) with fresh azimuths.
    Ai is Ae itself when opt.lambda_ic <= 0.  opt.beta > 0 raises, as the reference's trainer.py:322 does (a legacy
    ``torch.FloatTensor(ndarray, device='cuda')`` constructor)."""
    lam = opt.lambda_ic > 0.0
    if lam and opt.beta > 0:
        raise RuntimeError("opt.beta > 0: the reference's trainer.py:322 builds alpha with torch.FloatTensor(ndarray, device='cuda'), "
                           "which raises (legacy constructor expects device type: cpu); there is no result to reproduce")
    v = Ae["vertices"]
    N.require_device(v)
    B, dev = v.shape[0], v.device
    f32 = dict(dtype=torch.float32, device=dev)
    Ae90 = None
    if opt.hard:
        Ae90 = {k: val for k, val in Ae.items() if k in COPY_KEYS}
        if random.random() > 0.5:
            az = -torch.empty(B, **f32).uniform_(opt.hard_range, 180 - opt.hard_range)
        else:
            az = -torch.empty(B, **f32).uniform_(0, 180)
        r = torch.empty(B, **f32).uniform_(-1.0, 1.0)
        Ae90["azimuths"] = az * torch.where(r < 0, -1.0, 1.0)  # trainer.py:287-289's masked writes, without a nonzero()
    rand_a = np.random.permutation(B)
    rand_b = np.random.permutation(B)
    if not lam:
        return Ae, Ae90
    Ai = {}
    torch.empty(B, **f32).uniform_(0.0, 1.0)                    # alpha_camera: unused by the reference, drawn for the stream
    Ai["azimuths"] = -torch.empty(B, **f32).uniform_(-opt.azi_scope / 2, opt.azi_scope / 2)
    Ai["elevations"] = torch.empty(B, **f32).uniform_(elev_range[0], elev_range[1])
    Ai["distances"] = torch.empty(B, **f32).uniform_(dist_range[0], dist_range[1])
    Ai["biases"] = torch.empty((B, 2), **f32).uniform_(-opt.bias_range, opt.bias_range)
    alpha_texture = torch.empty((B, 1, 1, 1), **f32).uniform_(0.0, 1.0)
    alpha_shape = torch.empty((B, 1, 1), **f32).uniform_(0.0, 1.0)
    alpha_light = torch.empty((B, 1), **f32).uniform_(0.0, 1.0)
    ia, ib = rand_a, rand_b
    if opt.inv == 0:
        u = torch.empty((2, B), **f32).uniform_(0.0, 1.0, generator=generator)
        ia, ib, _ = resample_collapsed(Ae["delta_vertices"], rand_a, rand_b, u)
    A = {k: Ae[k] for k in ("vertices", "delta_vertices", "textures", "lights")}
    A["bg"] = Ae.get("bg") if opt.bg else None
    Ai.update(mix_attributes(A, ia, ib, alpha_shape, alpha_texture, alpha_light))
    return Ai, Ae90
