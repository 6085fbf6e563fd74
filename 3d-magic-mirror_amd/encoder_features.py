"""Template-anchored encoder features: host side of ``mm_shape_features_* / mm_camera_features_*`` (csrc/mm_encfeat.hip).

``shape_features(x, template, lpl, p)`` is the tensor the reference's ``ShapeEncoder.forward`` builds before ``encoder2``
(the reference's network/model_res.py:318-327, ``nolpl=False``):
``torch.cat((local, glob, neighbor_diff, xyz), 1).squeeze(3)`` of shape (B, 3C+3, V), where ``local`` samples the backbone map
at the template's (x, y) (bilinear, ``align_corners=True``, zero padding), ``glob`` is ``MMPool((1,1))`` (weight ``sigmoid(p)``
between the global max and mean) repeated over V, and ``neighbor_diff = local @ lpl`` with the dense (V,V) Laplacian, computed
from its non-zeros only.  ``camera_features(x, template, p_map, p_local)`` is ``CameraEncoder.forward``'s
``torch.cat((MMPool((2,2))(x), MMPool((2,2))(grid_sample(x, uv, align_corners=False))), 1)`` of shape (B, 2C, 2, 2).

``x`` may be fp32, fp16 or bf16 with any strides; outputs are fp32, ``x``'s gradient comes back in ``x``'s dtype.  The template
and ``lpl`` are constants (the reference detaches the template; an ``lpl`` that requires grad is refused).  Gradients reach
``x`` and the pool weights, atomic-free and bitwise reproducible.  Device tensors only."""
import collections
import weakref

import torch

from . import _native as N

_DTYPES = {torch.float32: N.DTYPE_F32, torch.float16: N.DTYPE_F16, torch.bfloat16: N.DTYPE_BF16}


# ---- lpl as two fixed-stride sparse tables, cached on the tensor's identity, address, version and shape ------------------------
def _ell_columns(m):
    """(idx (K,V) int32, val (K,V) float32) of the non-zeros of every COLUMN u of the (V,V) float32 host matrix m: rows v ascending
    at [k, u], padded with -1 / 0; K = the most non-zeros of any column (at least 1)."""
    nz = m != 0
    cnt = nz.sum(0)
    K = max(int(cnt.max()), 1)
    order = torch.sort((~nz).to(torch.int8), dim=0, stable=True).indices[:K]        # the non-zero rows first, in row order
    valid = torch.arange(K)[:, None] < cnt[None, :]
    idx = torch.where(valid, order, torch.full_like(order, -1)).to(torch.int32)
    val = torch.where(valid, m.gather(0, order), torch.zeros((), dtype=m.dtype))
    return idx.contiguous(), val.to(torch.float32).contiguous()


_LPL_CACHE = collections.OrderedDict()
_LPL_CACHE_SIZE = 8


def lpl_tables(lpl, device):
    """The column table (neighbor[u] = sum_k local[idx[k,u]] * val[k,u]) and the row table (the same for lpl^T, the backward's
    gather) of ``lpl`` on ``device``: (col_idx, col_val, row_idx, row_val).  Built once per (tensor, data_ptr, _version, shape,
    strides) -- an in-place edit, a ``.data`` reassignment or a new tensor is picked up -- with one device-to-host copy when
    ``lpl`` lives on the device.  Resident: the four uploads are blocking copies from pageable memory that have finished when this returns,
    and the tables are only read afterwards, so calls on any stream may share them."""
    key = (lpl.data_ptr(), lpl._version, tuple(lpl.shape), tuple(lpl.stride()), lpl.dtype, str(lpl.device), str(device))
    hit = _LPL_CACHE.get(key)
    if hit is not None and hit[0]() is lpl:
        _LPL_CACHE.move_to_end(key)
        return hit[1]
    m = lpl.detach().to(device="cpu", dtype=torch.float32)
    ci, cv = _ell_columns(m)
    ri, rv = _ell_columns(m.t())
    tables = tuple(t.to(device) for t in (ci, cv, ri, rv))
    _LPL_CACHE[key] = (weakref.ref(lpl), tables)
    while len(_LPL_CACHE) > _LPL_CACHE_SIZE:
        _LPL_CACHE.popitem(last=False)
    return tables


# ---- validation: every shape is checked here, before anything reaches a kernel -------------------------------------------------
def _check_x(x, what):
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError("%s expects x of shape (B,C,H,W), got %s" % (what, tuple(x.shape) if torch.is_tensor(x) else type(x)))
    if x.dtype not in _DTYPES:
        raise ValueError("%s expects x in float32, float16 or bfloat16, got %s" % (what, x.dtype))
    if min(x.shape) < 1:
        raise ValueError("%s expects a non-empty x, got shape %s" % (what, tuple(x.shape)))
    B, C, H, W = x.shape
    if B * C > 0x7fffffff or H * W > (1 << 30):
        raise ValueError("%s: x of shape %s is too large (B*C < 2^31, H*W <= 2^30)" % (what, tuple(x.shape)))


def _check_template(t, what):
    """V of a (1,V,3) or (V,3) template"""
    if not torch.is_tensor(t) or not (t.dim() == 2 or (t.dim() == 3 and t.shape[0] == 1)) or t.shape[-1] != 3 or t.shape[-2] < 1:
        raise ValueError("%s expects template of shape (1,V,3) or (V,3), got %s" % (what, tuple(t.shape) if torch.is_tensor(t) else type(t)))
    V = t.shape[-2]
    if V > N.ENCFEAT_MAX_V:
        raise ValueError("%s supports at most %d template vertices, got template of shape %s" % (what, N.ENCFEAT_MAX_V, tuple(t.shape)))
    return V


def _template_xy(t, dev):
    """the template as the kernels read it: (V,3) float32, dense, on dev (read afresh every call: in-place edits are seen)"""
    return t.detach().reshape(-1, 3).to(device=dev, dtype=torch.float32).contiguous()


def _check_p(p, name, what):
    if not torch.is_tensor(p) or p.numel() != 1:
        raise ValueError("%s expects %s with one element (MMPool.p), got %s" % (what, name, tuple(p.shape) if torch.is_tensor(p) else type(p)))


def _dev_scalar(p, dev):
    return p.detach().reshape(1).to(device=dev, dtype=torch.float32).contiguous()


def _like(g, p):
    """a p gradient computed as (1,) float32 on the device, in p's shape, dtype and device"""
    return None if g is None else g.to(device=p.device, dtype=p.dtype).reshape(p.shape)


def _fill_x(d, x):
    d.B, d.C, d.H, d.W = x.shape
    d.x_dtype = _DTYPES[x.dtype]
    d.x = N.ptr(x)
    for i, s in enumerate(x.stride()):
        d.x_strides[i] = s


# ---- shape features ---------------------------------------------------------------------------------------------------------------
def _shape_desc(x, tmpl, tables, p, out=None):
    d = N.MMShapeFeatDesc()
    _fill_x(d, x)
    d.V = tmpl.shape[0]
    d.template_xyz = N.ptr(tmpl)
    ci, cv, ri, rv = tables
    d.col_k, d.col_idx, d.col_val = ci.shape[0], N.ptr(ci), N.ptr(cv)
    d.row_k, d.row_idx, d.row_val = ri.shape[0], N.ptr(ri), N.ptr(rv)
    d.p = N.ptr(p)
    d.out = N.ptr(out)
    return d


def _shape_forward(x, tmpl, tables, p):
    B, C = x.shape[:2]
    out = torch.empty((B, 3 * C + 3, tmpl.shape[0]), device=x.device, dtype=torch.float32)
    d = _shape_desc(x, tmpl, tables, p, out)
    N.call("mm_shape_features_forward", x.device, d)
    return out


class _ShapeFeatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, tmpl, ci, cv, ri, rv):
        pd = _dev_scalar(p, x.device)
        out = _shape_forward(x, tmpl, (ci, cv, ri, rv), pd)
        ctx.save_for_backward(x, pd, tmpl, ci, cv, ri, rv)
        ctx.p_like = torch.empty(p.shape, dtype=p.dtype, device=p.device) if ctx.needs_input_grad[1] else None
        return out

    @staticmethod
    def backward(ctx, g):
        x, pd, tmpl, ci, cv, ri, rv = ctx.saved_tensors
        dev = x.device
        g = g.to(torch.float32).contiguous()
        gx = torch.empty(x.shape, device=dev, dtype=x.dtype) if ctx.needs_input_grad[0] else None
        gp = torch.empty(1, device=dev, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        d = _shape_desc(x, tmpl, (ci, cv, ri, rv), pd)
        ws = N.workspace("mm_shape_features_query_workspace", d, dev)
        gr = N.MMShapeFeatGrads(N.ptr(g), N.ptr(gx), N.ptr(gp))
        N.call("mm_shape_features_backward", dev, d, gr)
        return gx, _like(gp, ctx.p_like), None, None, None, None, None


def shape_features(x, template, lpl, p):
    """(B, 3C+3, V) float32 = cat(local, glob, neighbor_diff, xyz) of ShapeEncoder.forward (model_res.py:318-327).

    x: (B,C,H,W) backbone map (fp32 / fp16 / bf16, any strides); template: (1,V,3) or (V,3), columns 0 / 1 sample width / height
    (a constant); lpl: (V,V) on the host or the device (a constant; must not require grad); p: MMPool.p, one element."""
    what = "shape_features"
    _check_x(x, what)
    V = _check_template(template, what)
    if not torch.is_tensor(lpl) or tuple(lpl.shape) != (V, V):
        raise ValueError("%s expects lpl of shape (%d,%d) for a %d-vertex template, got %s" % (what, V, V, V, tuple(lpl.shape) if torch.is_tensor(lpl) else type(lpl)))
    if lpl.requires_grad:
        raise RuntimeError("%s treats lpl as a constant, but lpl (shape %s) requires grad" % (what, tuple(lpl.shape)))
    _check_p(p, "p", what)
    N.require_device(x)
    tmpl = _template_xy(template, x.device)
    tables = lpl_tables(lpl, x.device)
    if torch.is_grad_enabled() and (x.requires_grad or p.requires_grad):
        return _ShapeFeatFn.apply(x, p, tmpl, *tables)
    return _shape_forward(x, tmpl, tables, _dev_scalar(p, x.device))


# ---- camera features --------------------------------------------------------------------------------------------------------------
def _camera_desc(x, tmpl, pm, pl, out=None):
    d = N.MMCameraFeatDesc()
    _fill_x(d, x)
    d.V = tmpl.shape[0]
    d.template_xyz = N.ptr(tmpl)
    d.p_map, d.p_local = N.ptr(pm), N.ptr(pl)
    d.out = N.ptr(out)
    return d


def _camera_forward(x, tmpl, pm, pl):
    B, C = x.shape[:2]
    out = torch.empty((B, 2 * C, 2, 2), device=x.device, dtype=torch.float32)
    d = _camera_desc(x, tmpl, pm, pl, out)
    N.call("mm_camera_features_forward", x.device, d)
    return out


class _CameraFeatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p_map, p_local, tmpl):
        pm, pl = _dev_scalar(p_map, x.device), _dev_scalar(p_local, x.device)
        out = _camera_forward(x, tmpl, pm, pl)
        ctx.save_for_backward(x, pm, pl, tmpl)
        ctx.p_like = tuple(torch.empty(q.shape, dtype=q.dtype, device=q.device) for q in (p_map, p_local))
        return out

    @staticmethod
    def backward(ctx, g):
        x, pm, pl, tmpl = ctx.saved_tensors
        dev = x.device
        g = g.to(torch.float32).contiguous()
        need = ctx.needs_input_grad
        gx = torch.empty(x.shape, device=dev, dtype=x.dtype) if need[0] else None
        gpm = torch.empty(1, device=dev, dtype=torch.float32) if need[1] else None
        gpl = torch.empty(1, device=dev, dtype=torch.float32) if need[2] else None
        d = _camera_desc(x, tmpl, pm, pl)
        ws = N.workspace("mm_camera_features_query_workspace", d, dev)
        gr = N.MMCameraFeatGrads(N.ptr(g), N.ptr(gx), N.ptr(gpm), N.ptr(gpl))
        N.call("mm_camera_features_backward", dev, d, gr)
        return gx, _like(gpm, ctx.p_like[0]), _like(gpl, ctx.p_like[1]), None


def camera_features(x, template, p_map, p_local):
    """(B, 2C, 2, 2) float32 = cat(MMPool((2,2))(x), MMPool((2,2))(grid_sample(x, uv, align_corners=False))) of
    CameraEncoder.forward (model_res.py:198-200); the sampled (B,C,V,1) map is never materialised.

    x: (B,C,H,W) (fp32 / fp16 / bf16, any strides); template: (1,V,3) or (V,3), a constant; p_map, p_local: the two pools' p."""
    what = "camera_features"
    _check_x(x, what)
    _check_template(template, what)
    _check_p(p_map, "p_map", what)
    _check_p(p_local, "p_local", what)
    N.require_device(x)
    tmpl = _template_xy(template, x.device)
    if torch.is_grad_enabled() and (x.requires_grad or p_map.requires_grad or p_local.requires_grad):
        return _CameraFeatFn.apply(x, p_map, p_local, tmpl)
    return _camera_forward(x, tmpl, _dev_scalar(p_map, x.device), _dev_scalar(p_local, x.device))
