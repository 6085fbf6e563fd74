"""Multi-view rendering (DiffRender.render_views, MMRenderViewsDesc / mm_render_views_* of include/mm_render.h) without a GPU: the C ABI's
mirror, the argument checks of the three entry points (fake non-NULL pointers that are never dereferenced: every call must fail its
validation before any launch), the workspace arithmetic, and the Python API's shape validation."""
import ctypes
import importlib
import os

import pytest
import torch

from conftest import TEMPLATES

N = importlib.import_module("3d-magic-mirror_amd._native")

FAKE = 256                                                   # a 256-byte aligned non-NULL address nobody reads
NULL_POINTER, BAD_SHAPE, WORKSPACE, UNSUPPORTED = -1, -2, -3, -5
ENTRY = ("mm_render_views_query_workspace", "mm_render_views_forward", "mm_render_views_backward")


def test_abi_mirrors_the_new_struct_and_symbols(pkg):
    L = N.lib()
    assert N.ABI_VERSION == 9 == L.mm_abi_version()
    assert L.mm_struct_size(26) == ctypes.sizeof(N.MMRenderViewsDesc) > ctypes.sizeof(N.MMRenderDesc)
    assert L.mm_struct_size(0) == ctypes.sizeof(N.MMRenderDesc) and L.mm_struct_size(1) == ctypes.sizeof(N.MMRenderGrads)
    assert N.MMRenderViewsDesc.render.offset == 0 and N.MMRenderViewsDesc.views.offset == ctypes.sizeof(N.MMRenderDesc)
    for name in ENTRY:
        assert name in N.EXPORTS and hasattr(L, name), name


def _desc(images=8, views=2, H=64, W=64, V=642, F=1280, Ht=128, Wt=64, no_mask=1, backward=False):
    """a descriptor every check accepts up to the workspace: sizes, every pointer the direction needs (fake), no workspace yet"""
    vd = N.MMRenderViewsDesc()
    d = vd.render
    d.B, d.H, d.W, d.V, d.F, d.Ht, d.Wt, d.no_mask, d.knum = images, H, W, V, F, Ht, Wt, no_mask, 30
    d.sigmainv, d.boxlen, d.multiplier, d.eps = 7000.0, 0.02, 1000.0, 1e-8
    for f in ("faces", "face_uvs", "vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases", "rgba", "face_idx",
              "face_normals"):
        setattr(d, f, FAKE)
    if backward:
        d.vc_table, d.vc_stride = FAKE, 6
    vd.views = views
    return vd


def _with_workspace(vd, short=0, misalign=0):
    L = N.lib()
    vd.render.workspace = FAKE + misalign
    vd.render.workspace_bytes = L.mm_render_views_query_workspace(ctypes.byref(vd)) - short
    return vd


def _grads():
    g = N.MMRenderGrads()
    for f, _ in N.MMRenderGrads._fields_:
        setattr(g, f, FAKE)
    return g


def _call(vd, backward, grads=None):
    L = N.lib()
    if backward:
        return L.mm_render_views_backward(ctypes.byref(vd), ctypes.byref(grads if grads is not None else _grads()), None)
    return L.mm_render_views_forward(ctypes.byref(vd), None)


@pytest.mark.parametrize("backward", [False, True])
def test_entry_points_reject_bad_arguments_before_any_launch(pkg, backward):
    L = N.lib()
    assert L.mm_render_views_forward(None, None) == NULL_POINTER and L.mm_render_views_backward(None, None, None) == NULL_POINTER
    assert L.mm_render_views_query_workspace(None) == 0
    # views < 1, or an image count that is not a multiple of the views
    for views in (0, -3):
        vd = _with_workspace(_desc(views=2, backward=backward))
        vd.views = views
        assert _call(vd, backward) == BAD_SHAPE, views
        assert L.mm_render_views_query_workspace(ctypes.byref(vd)) == 0
    vd = _with_workspace(_desc(images=8, views=2, backward=backward))
    vd.views = 3
    assert _call(vd, backward) == BAD_SHAPE
    assert L.mm_render_views_query_workspace(ctypes.byref(vd)) == 0
    # workspace: missing, one byte short of the query, misaligned
    vd = _desc(backward=backward)
    assert _call(vd, backward) == WORKSPACE
    assert _call(_with_workspace(_desc(backward=backward), short=1), backward) == WORKSPACE
    assert _call(_with_workspace(_desc(backward=backward), misalign=64), backward) == WORKSPACE
    assert _call(_with_workspace(_desc(views=1, backward=backward), short=1), backward) == WORKSPACE
    # what check_render refuses for the B*N-image descriptor keeps its code
    for f in ("H", "W", "V", "F", "Ht", "Wt", "B"):
        vd = _with_workspace(_desc(backward=backward))
        setattr(vd.render, f, 0)
        assert _call(vd, backward) == BAD_SHAPE, f
    vd = _with_workspace(_desc(backward=backward)); vd.render.knum = 0
    assert _call(vd, backward) == UNSUPPORTED
    vd = _desc(backward=backward); vd.render.H = 65536
    assert _call(_with_workspace(vd), backward) == UNSUPPORTED
    for f in ("faces", "face_uvs", "vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases", "face_idx", "face_normals"):
        vd = _with_workspace(_desc(backward=backward))
        setattr(vd.render, f, None)
        assert _call(vd, backward) == NULL_POINTER, f
    if backward:
        vd = _with_workspace(_desc(backward=True)); vd.render.vc_table = None
        assert _call(vd, True) == NULL_POINTER
        vd = _with_workspace(_desc(backward=True)); vd.render.vc_stride = 0
        assert _call(vd, True) == BAD_SHAPE
        for f in ("grad_rgba", "grad_vertices", "grad_textures", "grad_lights", "grad_bg", "grad_azimuths", "grad_elevations", "grad_distances", "grad_biases"):
            g = _grads(); setattr(g, f, None)
            assert _call(_with_workspace(_desc(backward=True)), True, g) == NULL_POINTER, f
        assert L.mm_render_views_backward(ctypes.byref(_with_workspace(_desc(backward=True))), None, None) == NULL_POINTER
    else:
        vd = _with_workspace(_desc()); vd.render.rgba = None
        assert _call(vd, False) == NULL_POINTER
    # fused and deferred losses, geometry-only: out of scope over views
    for f, val in (("fused_gt", FAKE), ("fused_totals", FAKE), ("geometry_only", 1)):
        vd = _with_workspace(_desc(backward=backward))
        setattr(vd.render, f, val)
        assert _call(vd, backward) == UNSUPPORTED, f
    assert L.mm_last_error_detail().decode() == ""                   # nothing launched, nothing recorded


def test_workspace_sizes(pkg):
    L = N.lib()
    for images, H, W, V, F, Ht, Wt in ((8, 64, 64, 642, 1280, 128, 64), (96, 128, 128, 642, 1280, 256, 128), (6, 128, 64, 642, 1280, 64, 64)):
        one = _desc(images=images, views=1, H=H, W=W, V=V, F=F, Ht=Ht, Wt=Wt)
        base = L.mm_query_workspace(ctypes.byref(one.render))
        assert base > 0 and L.mm_render_views_query_workspace(ctypes.byref(one)) == base      # views = 1: the render's own workspace
        for views in (2, 3, images):
            if images % views:
                continue
            vd = _desc(images=images, views=views, H=H, W=W, V=V, F=F, Ht=Ht, Wt=Wt)
            q = L.mm_render_views_query_workspace(ctypes.byref(vd))
            assert q % 256 == 0
            staging = 4 * images * (V * 3 + 3 * Ht * Wt + 9 + 3 * H * W)                      # the four per-image gradient areas, in bytes
            assert q >= base + staging, (images, views, q, base, staging)
            assert q <= base + staging + 4 * 256                                               # ... each rounded up to 256 bytes, nothing more
    bad = _desc(); bad.render.Ht = 0
    assert L.mm_render_views_query_workspace(ctypes.byref(bad)) == 0


# ---- DiffRender.render_views: everything is validated before any device work -----------------------------------------------------------
@pytest.fixture(scope="module")
def dr(pkg):
    return pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), 16)


def _attrs(dr, pkg, B=3, n=2):
    att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, B, 16, 16, seed=5)
    att = {k: v for k, v in att.items() if torch.is_tensor(v)}
    att["azimuths"] = att["azimuths"][:, None] + torch.arange(n, dtype=torch.float32)[None] * 90.0
    return att


def test_render_views_wants_a_view_axis(pkg, dr):
    att = _attrs(dr, pkg)
    att["azimuths"] = att["azimuths"][:, 0]
    with pytest.raises(ValueError, match="no camera attribute carries a view axis"):
        dr.render_views(no_mask=True, **att)


def test_render_views_refuses_disagreeing_view_counts(pkg, dr):
    att = _attrs(dr, pkg, n=2)
    att["elevations"] = att["elevations"][:, None].expand(3, 5)
    with pytest.raises(ValueError, match="disagree on the number of views.*'azimuths': 2.*'elevations': 5"):
        dr.render_views(no_mask=True, **att)
    att = _attrs(dr, pkg, n=2)
    att["biases"] = att["biases"][:, None, :].expand(3, 4, 2)
    with pytest.raises(ValueError, match="disagree"):
        dr.render_views(no_mask=True, **att)


def test_render_views_refuses_a_wrong_batch(pkg, dr):
    for key, bad in (("azimuths", torch.zeros(4, 2)), ("distances", torch.zeros(2)), ("biases", torch.zeros(3, 2, 3)), ("biases", torch.zeros(4, 2)),
                     ("elevations", torch.zeros(3, 2, 1))):
        att = _attrs(dr, pkg)
        att[key] = bad
        with pytest.raises(ValueError, match=key + r" must be \(3,N"):
            dr.render_views(no_mask=True, **att)
    for key, bad, msg in (("textures", torch.zeros(6, 3, 32, 16), r"textures must be \(3,3,Ht,Wt\)"), ("lights", torch.zeros(6, 9), r"lights must be \(3,9\)"),
                          ("bg", torch.zeros(6, 3, 16, 16), r"bg must be \(3,3,16,16\)"), ("vertices", torch.zeros(3, 10, 3), r"vertices must be \(B,642,3\)")):
        att = _attrs(dr, pkg)
        att[key] = bad
        with pytest.raises(ValueError, match=msg):
            dr.render_views(no_mask=True, **att)
    att = _attrs(dr, pkg)
    att["lights"] = None
    with pytest.raises(TypeError, match="lights"):
        dr.render_views(no_mask=True, **att)


def test_render_views_needs_bg_under_no_mask(pkg, dr):
    att = _attrs(dr, pkg)
    att["bg"] = None
    with pytest.raises(TypeError, match="needs attributes\\['bg'\\]"):
        dr.render_views(no_mask=True, **att)
    del att["bg"]
    with pytest.raises(TypeError, match="needs attributes\\['bg'\\]"):
        dr.render_views(no_mask=True, **att)


def test_render_views_refuses_cpu_tensors_like_render(pkg, dr):
    att = _attrs(dr, pkg)
    with pytest.raises(RuntimeError, match="device memory"):
        dr.render_views(no_mask=True, **att)
    att["bg"] = None
    with pytest.raises(RuntimeError, match="device memory"):
        dr.render_views(no_mask=False, **att)
    with pytest.raises(RuntimeError, match="device memory"):         # the refusal render itself gives
        dr.render(no_mask=False, **{k: (v[:, 0] if k == "azimuths" else v) for k, v in att.items()})
