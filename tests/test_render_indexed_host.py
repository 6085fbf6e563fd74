"""Indexed rendering (DiffRender.render_indexed, MMRenderIndexedDesc / mm_render_indexed_* of include/mm_render.h) without a GPU: the grid
helper, the host validation of the index argument, the C ABI's mirror, and the workspace arithmetic and argument checks of the entry points
(fake non-NULL pointers that are never dereferenced: every call must fail its validation before any launch)."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import TEMPLATES

N = importlib.import_module("3d-magic-mirror_amd._native")

FAKE = 256                                                   # a 256-byte aligned non-NULL address nobody reads
NULL_POINTER, BAD_SHAPE, WORKSPACE, UNSUPPORTED = -1, -2, -3, -5
ENTRY = ("mm_render_indexed_query_workspace", "mm_render_indexed_forward", "mm_render_indexed_backward")


# ---- grid_index --------------------------------------------------------------------------------------------------------------------------
def test_grid_index_values(pkg):
    row, col = pkg.grid_index(3, 4)
    assert row.dtype == col.dtype == torch.int64 and row.device.type == "cpu"
    assert row.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    assert col.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3]
    # the reference's nested loop (show_rainbow2.py:376-399): for every texture i, the shapes 0..n-1 in order
    want = [(i, j) for i in range(7) for j in range(5)]
    row, col = pkg.grid_index(7, 5)
    assert list(zip(row.tolist(), col.tolist())) == want
    row, col = pkg.grid_index(1, 1)
    assert row.tolist() == [0] and col.tolist() == [0]
    for bad in ((0, 3), (3, 0), (-1, 2)):
        with pytest.raises(ValueError, match="grid_index"):
            pkg.grid_index(*bad)
    assert importlib.import_module("mm_amd").grid_index is pkg.grid_index          # the alias exports what is added


# ---- host validation of `index` ------------------------------------------------------------------------------------------------------------
ROWS = {"vertices": 3, "textures": 5, "lights": 1, "bg": 2}


def _index(M=6):
    return {"vertices": [0, 2, 1, 1, 0, 2][:M], "textures": torch.tensor([4, 0, 3, 3, 1, 0][:M]), "lights": np.zeros(M, dtype=np.int32),
            "bg": torch.tensor([1, 0, 1, 0, 1, 1][:M], dtype=torch.int32)}


def test_check_render_index_accepts_and_normalises(pkg):
    out = pkg.check_render_index(_index(), ROWS, 6)
    assert set(out) == set(ROWS)
    for k, v in out.items():
        assert v.dtype == torch.int64 and v.shape == (6,) and v.device.type == "cpu", k
    assert out["vertices"].tolist() == [0, 2, 1, 1, 0, 2] and out["textures"].tolist() == [4, 0, 3, 3, 1, 0]
    ident = pkg.check_render_index(None, {"vertices": 6, "textures": 6, "lights": 6}, 6)
    assert ident == {"vertices": None, "textures": None, "lights": None}
    mixed = pkg.check_render_index({"textures": [0] * 6}, {"vertices": 6, "textures": 1, "lights": 6}, 6)
    assert mixed["vertices"] is None and mixed["textures"].tolist() == [0] * 6


@pytest.mark.parametrize("name", ["vertices", "textures", "lights", "bg"])
def test_check_render_index_refuses_on_the_host(pkg, name):
    R = ROWS[name]
    idx = _index(); idx[name] = list(idx[name])[:5] if not torch.is_tensor(idx[name]) else idx[name][:5]
    with pytest.raises(ValueError, match=r"index\['%s'\] must hold 6 entries" % name):                 # wrong length
        pkg.check_render_index(idx, ROWS, 6)
    idx = _index(); idx[name] = [0, 0, -1, 0, 0, 0]
    with pytest.raises(ValueError, match=r"index\['%s'\]\[2\] = -1 is outside the %d rows" % (name, R)):   # negative entry
        pkg.check_render_index(idx, ROWS, 6)
    idx = _index(); idx[name] = torch.tensor([0, 0, 0, 0, R, 0])
    with pytest.raises(ValueError, match=r"index\['%s'\]\[4\] = %d is outside the %d rows" % (name, R, R)):   # entry equal to the row count
        pkg.check_render_index(idx, ROWS, 6)
    idx = _index(); del idx[name]
    with pytest.raises(ValueError, match=r"%s holds %d rows for 6 images and index\['%s'\] is missing" % (name, R, name)):   # identity with rows != M
        pkg.check_render_index(idx, ROWS, 6)


def test_check_render_index_refuses_unknown_names_and_floats(pkg):
    with pytest.raises(ValueError, match="index has no 'azimuths'"):
        pkg.check_render_index({"azimuths": [0] * 6}, ROWS, 6)
    idx = _index(); idx["textures"] = torch.zeros(6)
    with pytest.raises(ValueError, match="must hold integers"):
        pkg.check_render_index(idx, ROWS, 6)
    idx = _index(); idx["textures"] = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="must hold 6 entries"):
        pkg.check_render_index(idx, ROWS, 6)


@pytest.fixture(scope="module")
def dr(pkg):
    return pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), 16)


def _attrs(dr, pkg, M=6):
    """M cameras over 3 meshes, 5 textures, 1 light row, 2 backgrounds (CPU tensors: nothing here reaches the device)"""
    att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, max(M, 5), 16, 16, seed=5)
    att = {k: v for k, v in att.items() if torch.is_tensor(v)}
    out = {k: att[k][:M] for k in ("azimuths", "elevations", "distances", "biases")}
    out.update(vertices=att["vertices"][:3], textures=att["textures"][:5], lights=att["lights"][:1], bg=att["bg"][:2])
    return out


def test_render_indexed_validates_before_any_device_work(pkg, dr):
    att = _attrs(dr, pkg)
    with pytest.raises(RuntimeError, match="device memory"):          # everything valid: the refusal render itself gives for CPU tensors
        dr.render_indexed(no_mask=True, index=_index(), **att)
    idx = _index(); idx["textures"] = [0, 1, 2, 3, 4, 5]
    with pytest.raises(ValueError, match=r"index\['textures'\]\[5\] = 5 is outside the 5 rows"):
        dr.render_indexed(no_mask=True, index=idx, **att)
    idx = _index(); idx["vertices"] = [0, 1]
    with pytest.raises(ValueError, match="must hold 6 entries"):
        dr.render_indexed(no_mask=True, index=idx, **att)
    idx = _index(); del idx["lights"]
    with pytest.raises(ValueError, match="lights holds 1 rows for 6 images"):
        dr.render_indexed(no_mask=True, index=idx, **att)
    with pytest.raises(ValueError, match="vertices holds 3 rows for 6 images"):
        dr.render_indexed(no_mask=True, **att)                         # index=None: the identity everywhere (the first tensor that is short)
    idx = _index(); del idx["bg"]                                      # without no_mask the bg is not part of the call: its index is not asked for
    with pytest.raises(RuntimeError, match="device memory"):
        dr.render_indexed(no_mask=False, index=idx, **att)
    bad = dict(att); bad["bg"] = None
    with pytest.raises(TypeError, match="needs attributes\\['bg'\\]"):
        dr.render_indexed(no_mask=True, index=_index(), **bad)
    bad = dict(att); bad["elevations"] = att["elevations"][:4]
    with pytest.raises(ValueError, match="one value per image"):
        dr.render_indexed(no_mask=True, index=_index(), **bad)
    bad = dict(att); bad["lights"] = torch.zeros(1, 8)
    with pytest.raises(ValueError, match=r"lights must be \(R,9\)"):
        dr.render_indexed(no_mask=True, index=_index(), **bad)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_abi_mirrors_the_new_struct_and_symbols(pkg):
    L = N.lib()
    assert N.ABI_VERSION == 9 == L.mm_abi_version()                    # an addition only
    assert L.mm_struct_size(33) != 0
    assert L.mm_struct_size(33) == ctypes.sizeof(N.MMRenderIndexedDesc) > ctypes.sizeof(N.MMRenderDesc)
    assert L.mm_struct_size(0) == ctypes.sizeof(N.MMRenderDesc) and L.mm_struct_size(26) == ctypes.sizeof(N.MMRenderViewsDesc)
    assert L.mm_struct_size(31) == 0 and L.mm_struct_size(34) == 0
    D = N.MMRenderIndexedDesc
    assert D.render.offset == 0 and D.rows.offset == ctypes.sizeof(N.MMRenderDesc) and D.index.offset == D.rows.offset + 16
    assert D.backward.offset == D.index.offset + 32 and D.status_flag.offset == D.backward.offset + 8
    for name in ENTRY:
        assert name in N.EXPORTS and hasattr(L, name), name


def _desc(M=11, rows=(3, 5, 1, 2), H=64, W=64, V=642, F=1280, Ht=128, Wt=64, no_mask=1, backward=1, for_backward=False):
    """a descriptor every check accepts up to the workspace: sizes, every pointer the direction needs (fake), no workspace yet"""
    vd = N.MMRenderIndexedDesc()
    d = vd.render
    d.B, d.H, d.W, d.V, d.F, d.Ht, d.Wt, d.no_mask, d.knum = M, H, W, V, F, Ht, Wt, no_mask, 30
    d.sigmainv, d.boxlen, d.multiplier, d.eps = 7000.0, 0.02, 1000.0, 1e-8
    for f in ("faces", "face_uvs", "vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases", "rgba", "face_idx",
              "face_normals"):
        setattr(d, f, FAKE)
    if for_backward:
        d.vc_table, d.vc_stride = FAKE, 6
    for t in range(4):
        vd.rows[t] = rows[t]
        vd.index[t] = FAKE
    vd.backward = backward
    return vd


def _with_workspace(vd, short=0, misalign=0):
    vd.render.workspace = FAKE + misalign
    vd.render.workspace_bytes = N.lib().mm_render_indexed_query_workspace(ctypes.byref(vd)) - short
    return vd


def _grads():
    g = N.MMRenderGrads()
    for f, _ in N.MMRenderGrads._fields_:
        setattr(g, f, FAKE)
    return g


def _call(vd, backward, grads=None):
    L = N.lib()
    if backward:
        return L.mm_render_indexed_backward(ctypes.byref(vd), ctypes.byref(grads if grads is not None else _grads()), None)
    return L.mm_render_indexed_forward(ctypes.byref(vd), None)


def test_workspace_sizes(pkg):
    L = N.lib()
    q = lambda vd: L.mm_render_indexed_query_workspace(ctypes.byref(vd))
    for M, rows, H, W, V, F, Ht, Wt in ((11, (3, 5, 1, 2), 64, 64, 642, 1280, 128, 64), (96, (48, 48, 48, 48), 128, 128, 642, 1280, 256, 128),
                                        (1764, (7, 7, 7, 1764), 128, 64, 642, 1280, 64, 64)):
        kw = dict(M=M, rows=rows, H=H, W=W, V=V, F=F, Ht=Ht, Wt=Wt)
        fwd, bwd = _desc(backward=0, **kw), _desc(backward=1, **kw)
        base = L.mm_query_workspace(ctypes.byref(fwd.render))
        staging = 4 * M * (V * 3 + 3 * Ht * Wt + 9 + 3 * H * W)                               # the four per-image gradient areas, in bytes
        plan = 4 * (5 * M + sum(2 * r + 1 + M for r in rows))                                 # table; per tensor offsets, cursors, images
        assert base > 0 and q(fwd) % 256 == 0 and q(bwd) % 256 == 0
        assert base + plan <= q(fwd) <= base + plan + 13 * 256                                # forward only: the plan, no staging
        assert q(bwd) >= q(fwd) + staging                                                     # with a backward: at least the four staging areas more
        assert q(bwd) <= q(fwd) + staging + 4 * 256                                           # ... each rounded up to 256 bytes, nothing more
    for kw in (dict(M=65536), dict(rows=(65536, 5, 1, 2)), dict(rows=(3, 65536, 1, 2)), dict(rows=(3, 5, 65536, 2)), dict(rows=(3, 5, 1, 65536))):
        assert q(_desc(**kw)) == 0, kw                                                        # more than 65535 images or rows
    assert q(_desc(M=65535, rows=(65535, 65535, 65535, 65535), H=16, W=16, Ht=8, Wt=8)) > 0
    assert q(_desc(rows=(3, 5, 1, 65536), no_mask=0)) > 0                                     # (no bg in the call: its row count is not looked at)
    for kw in (dict(rows=(0, 5, 1, 2)), dict(rows=(3, 5, -1, 2)), dict(Ht=0), dict(M=0)):
        assert q(_desc(**kw)) == 0, kw
    assert L.mm_render_indexed_query_workspace(None) == 0


@pytest.mark.parametrize("backward", [False, True])
def test_entry_points_reject_bad_arguments_before_any_launch(pkg, backward):
    L = N.lib()
    mk = lambda **kw: _desc(for_backward=backward, **kw)
    assert L.mm_render_indexed_forward(None, None) == NULL_POINTER and L.mm_render_indexed_backward(None, None, None) == NULL_POINTER
    # limits and row counts
    assert _call(_with_workspace(mk(M=65536)), backward) == UNSUPPORTED
    for t in range(4):
        rows = [3, 5, 1, 2]; rows[t] = 65536
        assert _call(_with_workspace(mk(rows=tuple(rows))), backward) == UNSUPPORTED, t
        rows[t] = 0
        assert _call(_with_workspace(mk(rows=tuple(rows))), backward) == BAD_SHAPE, t
    # the identity needs a row per image
    for t in range(4):
        vd = _with_workspace(mk()); vd.index[t] = None
        assert _call(vd, backward) == BAD_SHAPE, t
        rows = [3, 5, 1, 2]; rows[t] = 11
        vd = _with_workspace(mk(rows=tuple(rows)), short=1); vd.index[t] = None
        assert _call(vd, backward) == WORKSPACE, t                                            # M rows: accepted up to the (short) workspace
    vd = _with_workspace(mk(no_mask=0), short=1); vd.index[3] = None; vd.rows[3] = 0          # no bg in the call: neither is looked at
    vd.render.bg = None
    assert _call(vd, backward) == WORKSPACE
    # workspace: missing, one byte short of the query, misaligned; a forward-only call has no backward
    assert _call(mk(), backward) == WORKSPACE
    assert _call(_with_workspace(mk(), short=1), backward) == WORKSPACE
    assert _call(_with_workspace(mk(), misalign=64), backward) == WORKSPACE
    assert _call(_with_workspace(mk(backward=0), short=1), backward) == WORKSPACE
    if backward:
        assert _call(_with_workspace(mk(backward=0)), True) == WORKSPACE
    # what check_render refuses for the M-image descriptor keeps its code
    for f in ("H", "W", "V", "F", "Ht", "Wt", "B"):
        vd = _with_workspace(mk()); setattr(vd.render, f, 0)
        assert _call(vd, backward) == BAD_SHAPE, f
    vd = _with_workspace(mk()); vd.render.knum = 0
    assert _call(vd, backward) == UNSUPPORTED
    for f in ("faces", "face_uvs", "vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases", "face_idx", "face_normals"):
        vd = _with_workspace(mk()); setattr(vd.render, f, None)
        assert _call(vd, backward) == NULL_POINTER, f
    if backward:
        vd = _with_workspace(mk()); vd.render.vc_table = None
        assert _call(vd, True) == NULL_POINTER
        for f in ("grad_rgba", "grad_vertices", "grad_textures", "grad_lights", "grad_bg", "grad_azimuths", "grad_elevations", "grad_distances", "grad_biases"):
            g = _grads(); setattr(g, f, None)
            assert _call(_with_workspace(mk()), True, g) == NULL_POINTER, f
        assert L.mm_render_indexed_backward(ctypes.byref(_with_workspace(mk())), None, None) == NULL_POINTER
    else:
        vd = _with_workspace(mk()); vd.render.rgba = None
        assert _call(vd, False) == NULL_POINTER
    # fused and deferred losses, geometry-only: refused exactly as mm_render_views_* refuses them
    for f, val in (("fused_gt", FAKE), ("fused_totals", FAKE), ("geometry_only", 1)):
        vd = _with_workspace(mk()); setattr(vd.render, f, val)
        assert _call(vd, backward) == UNSUPPORTED, f
    assert L.mm_last_error_detail().decode() == ""                   # nothing launched, nothing recorded
