"""Template-anchored encoder features (3d-magic-mirror_amd/encoder_features.py, csrc/mm_encfeat.hip) without a GPU: the C ABI's
mirror and argument checks, the Python API's validation, the lpl sparse tables and their cache, and the float64 restatement of the
reference (network/model_res.py: ShapeEncoder / CameraEncoder / MMPool) that tests/test_gpu_encoder_features.py measures against."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import TEMPLATES

EF = importlib.import_module("3d-magic-mirror_amd.encoder_features")
N = importlib.import_module("3d-magic-mirror_amd._native")
T = importlib.import_module("3d-magic-mirror_amd.template")


# ---- the reference in float64 (torch on the host) --------------------------------------------------------------------------------
def mmpool64(x, shape, p):
    w = torch.sigmoid(p.double())
    return F.adaptive_max_pool2d(x, shape) * w + F.adaptive_avg_pool2d(x, shape) * (1 - w)


def shape_ref(x, template, lpl, p):
    """model_res.py:318-327 (nolpl=False), every tensor in float64; x / p may require grad"""
    B = x.shape[0]
    t = template.detach().reshape(1, -1, 3).double()
    V = t.shape[1]
    pos = t.repeat(B, 1, 1).view(B, V, 1, 3)
    local = F.grid_sample(x, pos[:, :, :, 0:2], mode="bilinear", align_corners=True, padding_mode="zeros")
    glob = mmpool64(x, (1, 1), p).repeat(1, 1, V, 1)
    nd = torch.mm(local.reshape(-1, V), lpl.double()).view(B, -1, V, 1)
    return torch.cat((local, glob, nd, pos.permute(0, 3, 1, 2)), dim=1).squeeze(3)


def camera_ref(x, template, p_map, p_local):
    """model_res.py:196-200, every tensor in float64"""
    B = x.shape[0]
    t = template.detach().reshape(1, -1, 3).double()
    V = t.shape[1]
    uv = t.repeat(B, 1, 1).view(B, V, 1, 3)[:, :, :, 0:2]
    local = F.grid_sample(x, uv, mode="bilinear", align_corners=False)
    return torch.cat((mmpool64(x, (2, 2), p_map), mmpool64(local, (2, 2), p_local)), dim=1)


def template_lpl(name):
    z = np.load(os.path.join(TEMPLATES, name + ".npz"))
    v = T.normalize_template(torch.from_numpy(z["vertices"]), 1)
    return v[None].float(), T.uniform_laplacian(v.shape[0], torch.from_numpy(z["faces"]).long()).float()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_mirrors_the_new_structs_and_symbols(pkg):
    L = N.lib()
    assert N.ABI_VERSION == 9 == L.mm_abi_version()
    for i, cls in zip(range(20, 24), (N.MMShapeFeatDesc, N.MMShapeFeatGrads, N.MMCameraFeatDesc, N.MMCameraFeatGrads)):
        assert L.mm_struct_size(i) == ctypes.sizeof(cls) > 0, cls.__name__
    for name in ("mm_shape_features_query_workspace", "mm_shape_features_forward", "mm_shape_features_backward",
                 "mm_camera_features_query_workspace", "mm_camera_features_forward", "mm_camera_features_backward"):
        assert name in N.EXPORTS and hasattr(L, name), name


def _shape_desc(B=2, C=3, H=4, W=4, V=10, k=1):
    d = N.MMShapeFeatDesc()
    d.B, d.C, d.H, d.W, d.V, d.x_dtype, d.col_k, d.row_k = B, C, H, W, V, N.DTYPE_F32, k, k
    return d


def test_entry_points_reject_bad_descriptors_before_any_launch(pkg):
    L = N.lib()
    fake = ctypes.c_void_p(16)                    # never dereferenced: every call below must fail validation first
    assert L.mm_shape_features_forward(None, None) == -1 and L.mm_camera_features_forward(None, None) == -1
    assert L.mm_shape_features_forward(ctypes.byref(N.MMShapeFeatDesc()), None) == -2
    assert L.mm_camera_features_forward(ctypes.byref(N.MMCameraFeatDesc()), None) == -2
    assert L.mm_shape_features_query_workspace(ctypes.byref(N.MMShapeFeatDesc())) == 0
    d = _shape_desc()
    assert L.mm_shape_features_query_workspace(ctypes.byref(d)) % 256 == 0 and L.mm_shape_features_query_workspace(ctypes.byref(d)) > 0
    assert L.mm_shape_features_forward(ctypes.byref(d), None) == -1                      # shape fine, pointers missing
    for field, bad in (("V", N.ENCFEAT_MAX_V + 1), ("V", 0), ("x_dtype", 3), ("col_k", 0), ("col_k", 11), ("row_k", 0), ("H", -1)):
        e = _shape_desc()
        setattr(e, field, bad)
        e.x = e.template_xyz = e.col_idx = e.col_val = e.row_idx = e.row_val = e.p = e.out = fake
        assert L.mm_shape_features_forward(ctypes.byref(e), None) == -2, (field, bad)
        assert L.mm_shape_features_query_workspace(ctypes.byref(e)) == 0
    e = _shape_desc(B=1 << 16, C=1 << 15)                                                 # B*C >= 2^31
    assert L.mm_shape_features_query_workspace(ctypes.byref(e)) == 0
    # the backward: gradients required, then the workspace
    d.x = d.template_xyz = d.col_idx = d.col_val = d.row_idx = d.row_val = d.p = fake
    assert L.mm_shape_features_backward(ctypes.byref(d), None, None) == -1
    g = N.MMShapeFeatGrads(fake, None, None)
    assert L.mm_shape_features_backward(ctypes.byref(d), ctypes.byref(g), None) == -1     # neither grad_x nor grad_p
    g.grad_p = fake
    assert L.mm_shape_features_backward(ctypes.byref(d), ctypes.byref(g), None) == -3     # no workspace
    d.workspace, d.workspace_bytes = fake, L.mm_shape_features_query_workspace(ctypes.byref(d)) - 1
    assert L.mm_shape_features_backward(ctypes.byref(d), ctypes.byref(g), None) == -3
    c = N.MMCameraFeatDesc()
    c.B, c.C, c.H, c.W, c.V, c.x_dtype = 2, 3, 1, 3, 7, N.DTYPE_BF16
    assert L.mm_camera_features_query_workspace(ctypes.byref(c)) > L.mm_shape_features_query_workspace(ctypes.byref(_shape_desc(2, 3, 1, 3, 7))) - 256
    assert L.mm_camera_features_forward(ctypes.byref(c), None) == -1
    c.x = c.template_xyz = c.p_map = c.p_local = fake
    cg = N.MMCameraFeatGrads(fake, None, None, None)
    assert L.mm_camera_features_backward(ctypes.byref(c), ctypes.byref(cg), None) == -1
    cg.grad_p_local = fake
    assert L.mm_camera_features_backward(ctypes.byref(c), ctypes.byref(cg), None) == -3
    c.W = 0
    assert L.mm_camera_features_backward(ctypes.byref(c), ctypes.byref(cg), None) == -2
    assert L.mm_camera_features_query_workspace(ctypes.byref(c)) == 0


# ---- the Python API's validation (all of it before the device check: these run on host tensors) ------------------------------------
def test_bad_shapes_raise_naming_the_shape(pkg):
    x = torch.zeros(2, 3, 4, 4)
    t, lpl, p = torch.zeros(1, 5, 3), torch.zeros(5, 5), torch.zeros(1)
    cases = [((torch.zeros(2, 3, 4), t, lpl, p), "(2, 3, 4)"), ((x, torch.zeros(2, 5, 3), lpl, p), "(2, 5, 3)"),
             ((x, torch.zeros(5, 2), lpl, p), "(5, 2)"), ((x, t, torch.zeros(5, 4), p), "(5, 4)"), ((x, t, lpl, torch.zeros(2)), "(2,)"),
             ((torch.zeros(2, 0, 4, 4), t, lpl, p), "(2, 0, 4, 4)"), ((x, torch.zeros(1, N.ENCFEAT_MAX_V + 1, 3), lpl, p), str(N.ENCFEAT_MAX_V + 1)),
             ((x.to(torch.float64), t, lpl, p), "float64")]
    for args, text in cases:
        with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)")):
            pkg.shape_features(*args)
    with pytest.raises(ValueError, match=r"\(2, 5, 3\)"):
        pkg.camera_features(x, torch.zeros(2, 5, 3), p, p)
    with pytest.raises(ValueError, match="p_local"):
        pkg.camera_features(x, t, p, torch.zeros(3))
    with pytest.raises(RuntimeError, match="requires grad"):
        pkg.shape_features(x, t, lpl.clone().requires_grad_(), p)
    with pytest.raises(RuntimeError, match="device memory"):          # valid shapes on the host: no fallback
        pkg.shape_features(x, t, lpl, p)
    with pytest.raises(RuntimeError, match="device memory"):
        pkg.camera_features(x, t, p, p)


# ---- lpl as sparse tables --------------------------------------------------------------------------------------------------------
def _apply_cols(idx, val, local):
    """sum_k local[..., idx[k,u]] * val[k,u] in float64 (padding: idx -1, val 0)"""
    idx = idx.long()
    g = local.double()[..., idx.clamp(min=0)]                          # (..., K, V)
    return (g * torch.where(idx >= 0, val.double(), torch.zeros((), dtype=torch.float64))).sum(-2)


@pytest.mark.parametrize("kind", ["sphere", "smpl_uv_642", "random_sparse", "dense", "zero", "one_column"])
def test_lpl_tables_equal_the_dense_product_in_float64(pkg, kind):
    g = torch.Generator().manual_seed(3)
    if kind in ("sphere", "smpl_uv_642"):
        _, lpl = template_lpl(kind)
    elif kind == "random_sparse":
        lpl = torch.randn(300, 300, generator=g) * (torch.rand(300, 300, generator=g) < 0.02)
    elif kind == "dense":
        lpl = torch.randn(97, 97, generator=g)
    elif kind == "zero":
        lpl = torch.zeros(13, 13)
    else:
        lpl = torch.zeros(40, 40)
        lpl[:, 7] = torch.randn(40, generator=g)
    V = lpl.shape[0]
    ci, cv, ri, rv = EF.lpl_tables(lpl, torch.device("cpu"))
    assert ci.dtype == ri.dtype == torch.int32 and cv.dtype == rv.dtype == torch.float32
    assert ci.shape[1] == ri.shape[1] == V and ci.shape[0] == max(int((lpl != 0).sum(0).max()), 1)
    local = torch.randn(5, V, generator=g, dtype=torch.float64)
    ref = local @ lpl.double()
    assert torch.allclose(_apply_cols(ci, cv, local), ref, rtol=1e-12, atol=1e-12)
    refT = local @ lpl.double().t()                                    # the backward's row gather
    assert torch.allclose(_apply_cols(ri, rv, local), refT, rtol=1e-12, atol=1e-12)
    # entries of a column are in row order, padding last
    for u in range(0, V, max(V // 7, 1)):
        rows = ci[:, u][ci[:, u] >= 0]
        assert torch.equal(rows.long(), torch.nonzero(lpl[:, u]).flatten())


def test_lpl_cache_follows_version_identity_and_address(pkg):
    dev = torch.device("cpu")
    _, lpl = template_lpl("sphere")
    a = EF.lpl_tables(lpl, dev)
    assert EF.lpl_tables(lpl, dev) is a                                 # cached
    lpl[3, 5] = 0.25                                                   # in-place edit: _version moves
    b = EF.lpl_tables(lpl, dev)
    assert b is not a and _apply_cols(b[0], b[1], torch.eye(642, dtype=torch.float64))[3, 5] == 0.25
    assert EF.lpl_tables(lpl, dev) is b
    new = lpl.clone()
    new[0, 1] = 7.0
    lpl.data = new                                                     # .data reassignment: new address
    c = EF.lpl_tables(lpl, dev)
    assert c is not b and _apply_cols(c[0], c[1], torch.eye(642, dtype=torch.float64))[0, 1] == 7.0
    other = lpl.clone()                                                # a different tensor with equal contents
    assert EF.lpl_tables(other, dev) is not c
    view = lpl[:, :]                                                   # a view shares the version counter: editing the base reaches it
    v0 = EF.lpl_tables(view, dev)
    lpl.mul_(2)
    assert EF.lpl_tables(view, dev) is not v0
