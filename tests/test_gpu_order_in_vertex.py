"""The tile sort inside the vertex launch (csrc/mm_vertex.hip: the order workgroups) against the sort in a launch of its own
(order_kernel, forced by MM_OPT_ORDER_LAUNCH): the first counts a tile's candidates from face boxes it recomputes, the second popcounts
the bin masks the record workgroups wrote.  The counts must be EQUAL -- a tile wrongly counted empty is never walked, and the number of
heavy tiles picks the cooperative walk -- so every case runs forward + fused loss + backward through the C ABI twice, once as the library
chooses and once with the bit, and requires, bit for bit (int32 views), the image, face_idx, the face normals, imnormal, the loss and all
eight gradients, and equal `nheavy` pairs {tiles walked cooperatively, tiles not empty} read back from the workspace
(mm_debug_step_layout).  Both workspaces are filled with a byte pattern first: a sort that wrote nothing cannot pass on what an earlier
case left in the allocator's memory.

The hand-made meshes replace the template of a DiffRender (faces, uvs, vertex-corner table) after it has loaded a committed one: the
template statistics the class derives (Laplacian, flip pairs) are not read by the render path."""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import TEMPLATES
from test_gpu_fused_step import _arrays, _bits, _same, _tile_counts
from test_step_plan_host import gen_dir, template_path  # noqa: F401  (gen_dir: the fixture the generated template is written under)

pytestmark = pytest.mark.gpu

HEAVY_CAND = 192                      # MM_HEAVY_CAND (csrc/mm_order.h): candidates from which a tile is walked by four waves together


def _native():
    return importlib.import_module("3d-magic-mirror_amd._native")


def _render(pkg, name, S, ratio=1, mesh=None, gen=None):
    """a DiffRender of a committed (or, with gen, generated) template; mesh = (vertices (V,3), faces (F,3)): that mesh in its place"""
    template = importlib.import_module("3d-magic-mirror_amd.template")
    dr = pkg.DiffRender(template_path(gen, name) if gen is not None else os.path.join(TEMPLATES, name + ".npz"), S, ratio=ratio, emit_imnormal=True)
    if mesh is not None:
        v, f = np.asarray(mesh[0], np.float32), np.asarray(mesh[1], np.int64)
        dr.vertices_init, dr.faces = torch.from_numpy(v), torch.from_numpy(f)
        dr.num_vertices, dr.num_faces = v.shape[0], f.shape[0]
        g = torch.Generator(device="cpu").manual_seed(7)
        dr.face_uvs = 0.1 + 0.8 * torch.rand(1, f.shape[0], 3, 2, generator=g)
        dr._vc_table = template.vertex_corner_table(dr.num_vertices, dr.faces)
        dr._static_cache.clear(); dr._desc_cache.clear()
    return dr


def _batch(pkg, dr, B, seed, exact_vertices=False, **cams):
    """synthetic inputs for dr; exact_vertices: the mesh as given (no noise); cams: per-image lists that replace the drawn cameras"""
    att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, B, dr.render_height, dr.image_size, seed=seed)
    if exact_vertices:
        att["vertices"] = dr.vertices_init[None].repeat(B, 1, 1).contiguous()
    for k, v in cams.items():
        att[k] = torch.tensor(v, dtype=torch.float32)
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    gt = gt.clone()
    gt[:, 3] = torch.rand(B, dr.render_height, dr.image_size, generator=g)    # (a mask without structure: every covered pixel has a gradient)
    return att, gt


def _both(pkg, dr, att, gt, no_mask=True, step_mode=True):
    """the step with the library's choice and with MM_OPT_ORDER_LAUNCH; returns (arrays, nheavy pairs (B,2)) after holding the two equal"""
    N, stepmod = _native(), importlib.import_module("3d-magic-mirror_amd.step")
    dev = torch.device("cuda:0")
    att = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in att.items()}
    gt = gt.to(dev)
    out = []
    for options in (0, N.OPT_ORDER_LAUNCH):
        dr.options = options
        st = stepmod.RenderLossStep(dr, att, gt, no_mask=no_mask, emit_imnormal=True, fused=True, step_mode=step_mode)
        assert st.d.options == options
        st.ws.fill_(0xAB)
        out.append(st)
    dr.options = 0
    new, old = out
    assert new.step_mode_taken() == old.step_mode_taken() == bool(step_mode)   # the bit has no say in step mode; every shape here is one it covers
    new.run(); old.run()
    a, b = _arrays(new), _arrays(old)
    _same(a, b)
    cn, co = _tile_counts(new)[:, :2], _tile_counts(old)[:, :2]
    assert np.array_equal(cn, co), "nheavy pairs differ: in the vertex launch %s, in its own launch %s" % (cn.tolist(), co.tolist())
    ntile = 4 * (-(-dr.render_height // 16)) * (-(-dr.image_size // 16))
    assert (cn >= 0).all() and (cn[:, 0] <= 32).all() and (cn[:, 1] <= ntile).all()
    return a, cn


# ---- ragged screen -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_mask,step_mode", [(True, True), (False, True), (True, False)])
def test_ragged_screen(pkg, no_mask, step_mode):
    """B=3, 40x24: partial last bins in both directions, a partial 16x16 block, tile slots outside the image (key 0, flagged empty).
    Once without step mode: the forward that leaves the pixel pass to the backward takes its tile order from the same place."""
    dr = _render(pkg, "sphere", 40, ratio=0.6)
    assert (dr.render_height, dr.image_size) == (24, 40)
    att, gt = _batch(pkg, dr, 3, seed=21)
    a, cn = _both(pkg, dr, att, gt, no_mask=no_mask, step_mode=step_mode)
    assert (a["face_idx"] >= 0).any() and (a["face_idx"] < 0).any() and (cn[:, 1] > 0).all()
    assert float(a["grad_vertices"].abs().max()) > 0 and float(a["grad_textures"].abs().max()) > 0


# ---- bin borders -------------------------------------------------------------------------------------------------------------------
def _border_mesh(D, W):
    """Two-pixel triangles at z = 0, camera on the z axis at distance D, W x W screen.  One sweep of 72 along x, one of 72 along y, each
    moving a quarter of a pixel per face over 18 pixels: a face's box ends are integer pixel indices (pixel_range), and a sweep longer than
    two bins in steps below one pixel takes both ends of the boxes through every index of a bin period -- 8k - 1, 8k and 8k + 1 among them,
    wherever rounding puts the thresholds.  Then three faces whose boxes are special: one far off screen (no bin), one wholly behind the
    camera plane, one with a corner ON the camera plane (a division by zero: pixel_range's "every pixel" branch).  147 faces: three mask
    words, the last one partial."""
    px = 2.0 * D / (2.5 * W)                                     # world units per pixel at z = 0 (the projection is 2.5 x / z)
    v, f = [], []

    def tri(x, y, z=0.0, s=2.0 * px):
        n = len(v)
        v.extend([(x, y, z), (x + s, y, z), (x, y + s, z)])
        f.append((n, n + 1, n + 2))
    for k in range(72):
        tri(-9.0 * px + 0.25 * px * k, 3.1 * px)
        tri(-5.3 * px, -9.0 * px + 0.25 * px * k)
    tri(40.0 * W * px, 0.0)
    tri(0.0, 0.0, z=D + 1.0)
    n = len(v)
    v.extend([(0.0, 0.0, D), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0)])
    f.append((n, n + 1, n + 2))
    return np.array(v, np.float32), np.array(f, np.int64)


def test_bin_borders(pkg):
    D, W = 5.0, 64
    dr = _render(pkg, "sphere", W, mesh=_border_mesh(D, W))
    assert dr.num_faces == 147 and dr.num_faces % 64 != 0
    # the camera on the axis, then a little closer and turned by a fraction of a degree: the same sweeps on other thresholds
    att, gt = _batch(pkg, dr, 3, seed=31, exact_vertices=True, azimuths=[0.0, 0.0, 0.3], elevations=[0.0, 0.0, 0.2], distances=[D, D - 0.013, D],
                     biases=[[0.0, 0.0]] * 3)
    a, cn = _both(pkg, dr, att, gt)
    ntile = 4 * 16
    assert (cn[:, 1] > 4).all() and (cn[:, 1] <= ntile).all()    # the sweeps touch a band of tiles (and the corner on the camera plane may touch all)


# ---- an empty image beside a normal one ------------------------------------------------------------------------------------------------
def test_empty_image(pkg):
    dr = _render(pkg, "sphere", 32)
    att, gt = _batch(pkg, dr, 2, seed=33)
    att["vertices"][0, :, 0] += 100.0                             # image 0: the whole mesh far to the side of every camera the batch draws
    a, cn = _both(pkg, dr, att, gt)
    assert cn[0].tolist() == [0, 0] and cn[1, 1] > 0
    assert bool((a["face_idx"][0] < 0).all()) and bool((a["face_idx"][1] >= 0).any())


# ---- the cooperative branch ------------------------------------------------------------------------------------------------------------
def test_cooperative_walk_is_taken(pkg):
    """smpl_uv_642 (1 280 faces: five per thread of the order workgroup) at 64x64 from distances 10 and 16: the mesh is 16 and 10 pixels
    across, so its faces' boxes fall into at most 3x3 tiles and the middle one holds far more than 192 of them."""
    dr = _render(pkg, "smpl_uv_642", 64)
    assert dr.num_faces == 1280
    att, gt = _batch(pkg, dr, 2, seed=35, distances=[10.0, 16.0])
    a, cn = _both(pkg, dr, att, gt)
    print("tile counts {cooperative, non-empty}:", cn.tolist())
    assert (cn[:, 0] >= 1).all(), "no tile with %d candidates: the cooperative walk was not taken (%s)" % (HEAVY_CAND, cn.tolist())
    assert (cn[:, 1] < 32).all() and (a["face_idx"] >= 0).any(dim=2).any(dim=1).all()


# ---- close-up --------------------------------------------------------------------------------------------------------------------------
def test_close_up_faces_cover_every_bin(pkg):
    """Three faces (fewer than a wave), each larger than the 128x128 screen: every face's bin range is the whole 16x16 grid, the difference
    array's one entry at (0, 0) must reach every bin, and every tile's count is 3."""
    big = 40.0
    v = np.array([(-big, -big, 0.0), (big, -big, 0.0), (0.0, big, 0.0),
                  (-big, -big, -0.5), (big, -big, -0.5), (0.0, big, -0.5),
                  (-big, big, -1.0), (0.0, -big, -1.0), (big, big, -1.0)], np.float32)
    f = np.array([(0, 1, 2), (3, 4, 5), (6, 7, 8)], np.int64)
    dr = _render(pkg, "sphere", 128, mesh=(v, f))
    att, gt = _batch(pkg, dr, 2, seed=37, exact_vertices=True, azimuths=[0.0, 0.0], elevations=[0.0, 0.0], distances=[3.0, 4.0],
                     biases=[[0.0, 0.0], [0.1, -0.1]])             # (cameras on the axis: every corner stays in front of the camera plane)
    a, cn = _both(pkg, dr, att, gt)
    assert cn.tolist() == [[0, 256], [0, 256]]


# ---- two passes of the face loop -------------------------------------------------------------------------------------------------------
def test_sixteen_faces_per_thread(pkg, gen_dir):
    """The 4 096-face lat-long sphere: the largest mesh the predicate takes (64 mask words), two passes of eight faces per thread"""
    dr = _render(pkg, "latlong4096", 48, gen=gen_dir)
    assert dr.num_faces == 4096
    att, gt = _batch(pkg, dr, 2, seed=39)
    a, cn = _both(pkg, dr, att, gt)
    assert (cn[:, 1] > 0).all() and (a["face_idx"] >= 0).any()


# ---- shapes the predicate leaves alone -------------------------------------------------------------------------------------------------
def test_excluded_calls_run_unchanged(pkg):
    """A geometry_only call (no screen pass: no tile order) and a two-view render_views call (the *_views kernels, which carry no order
    workgroups) succeed and agree with and without the bit; their results are the existing suites' business."""
    N = _native()
    dev = torch.device("cuda:0")
    dr = _render(pkg, "sphere", 32)
    att, _ = _batch(pkg, dr, 2, seed=41)
    att = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in att.items()}
    got = []
    for options in (0, N.OPT_ORDER_LAUNCH):
        dr.options = options
        geo = dr.render_geometry(**dict(att))["face_normals"]
        cams = {k: att[k][:, None].repeat(1, 2, *([1] * (att[k].dim() - 1))) for k in ("azimuths", "elevations", "distances", "biases")}
        cams["azimuths"] = cams["azimuths"] + torch.tensor([0.0, 90.0], device=dev)
        rgbs, out = dr.render_views(**{**att, **cams})
        torch.cuda.synchronize()
        got.append((geo.clone(), rgbs.clone(), dr.last_face_idx.clone()))
    dr.options = 0
    for x, y in zip(*got):
        assert torch.equal(_bits(x), _bits(y))
    assert got[0][1].shape[:2] == (2, 2) and bool((got[0][2] >= 0).any())
