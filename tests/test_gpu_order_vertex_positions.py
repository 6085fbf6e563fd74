"""The order workgroup's boxes on meshes whose faces SHARE vertices in unusual ways, its face loads at the edges of a pass, and its
wave-parallel scans (csrc/mm_vertex.hip, order_workgroup).

The cases were drawn up for an order workgroup that forms the screen position of every VERTEX once and keeps it in LDS.  That form was
built, held these cases, and measured slower than forming every corner (profiles/order_vertex_positions_ab.md), so the workgroup still
transforms per face -- but it now loads a pass's corner ids from clamped addresses (past the mesh's end a lane reads the last face again
and skips it) and scans the bins with DPP steps, 16, 32 or 64 lanes per line.  The cases stay: they are what a per-vertex phase must hold
if it is tried again, and they pin what did change.  Every case is tests/test_gpu_order_in_vertex.py's comparison (_both: forward +
fused loss + backward with and without MM_OPT_ORDER_LAUNCH; every output, every gradient and every `nheavy` pair equal bit for bit):
a vertex that is every face's corner, vertices no face names, face counts around a row of threads (256) and around a pass (1 024),
shared vertices on and behind the camera plane, and bin grids at each width of the scans."""
import os

import numpy as np
import pytest
import torch

from test_gpu_loss_kernels_edges import _write_template
from test_gpu_order_in_vertex import _batch, _both, _render
from test_step_plan_host import gen_dir  # noqa: F401  (the fixture the generated template is written under)

pytestmark = pytest.mark.gpu


def _fan(V):
    """a cone: vertex 0 is a corner of every one of the V - 1 faces around it"""
    n = V - 1
    t = 2.0 * np.pi * np.arange(n) / n
    v = np.concatenate([[(0.0, 0.0, 0.5)], np.stack([0.9 * np.cos(t), 0.9 * np.sin(t), np.zeros(n)], 1)]).astype(np.float32)
    f = np.array([(0, 1 + i, 1 + (i + 1) % n) for i in range(n)], np.int64)
    return v, f


def _bipyramid(V):
    """a closed double cone: two apexes over a ring of V - 2 vertices, 2 (V - 2) faces wound outwards"""
    n = V - 2
    t = 2.0 * np.pi * np.arange(n) / n
    v = np.concatenate([[(0.0, 1.0, 0.0)], np.stack([np.cos(t), np.zeros(n), np.sin(t)], 1), [(0.0, -1.0, 0.0)]]).astype(np.float32)
    f = [(0, 1 + (i + 1) % n, 1 + i) for i in range(n)] + [(n + 1, 1 + i, 1 + (i + 1) % n) for i in range(n)]
    return v, np.array(f, np.int64)


def _all_finite(a):
    for k, x in a.items():
        if torch.is_tensor(x) and x.is_floating_point():
            assert bool(torch.isfinite(x).all()), k


# ---- one vertex in every face; face counts around a row of threads and around a pass ------------------------------------------------------
@pytest.mark.parametrize("V", [201, 256, 257, 258, 1024, 1026])
def test_fan(pkg, V):
    """V = 201: the fan of 200 faces.  F = V - 1 = 255, 256, 257: the first row of 256 threads one short, full, and one face in the second
    row (whose other lanes read the last face from a clamped address and skip it).  F = 1 023 and 1 025: the same around a whole pass of
    four rows -- one face short of it, and one face in a second pass."""
    v, f = _fan(V)
    assert f.shape[0] == V - 1 and (f == 0).any(axis=1).all()
    dr = _render(pkg, "sphere", 64, mesh=(v, f))
    att, gt = _batch(pkg, dr, 2, seed=51)
    a, cn = _both(pkg, dr, att, gt)
    assert (cn[:, 1] > 0).all() and (a["face_idx"] >= 0).any()
    assert float(a["grad_vertices"][:, 0].abs().max()) > 0          # the shared vertex takes gradient


@pytest.mark.parametrize("V", [258, 514])
def test_full_rows_of_faces(pkg, V):
    """F = 512 (two full rows of 256 faces; V = 258 is no multiple of 64) and F = 1 024 (exactly one pass): no lane past the end, two apexes
    shared by half the faces each"""
    v, f = _bipyramid(V)
    assert f.shape[0] == 2 * (V - 2) and f.shape[0] % 256 == 0
    dr = _render(pkg, "sphere", 48, mesh=(v, f))
    att, gt = _batch(pkg, dr, 2, seed=53)
    a, cn = _both(pkg, dr, att, gt)
    assert (cn[:, 1] > 0).all() and (a["face_idx"] >= 0).any()


def test_generated_template_second_pass_partial(pkg, gen_dir):
    """A generated closed template of 768 vertices and 1 532 faces: a second pass of which two rows are partly or wholly past the end"""
    V = 768
    v, f = _bipyramid(V)
    path = _write_template(os.path.join(str(gen_dir), "bipyramid%d.npz" % V), v, f)
    dr = pkg.DiffRender(path, 48, emit_imnormal=True)
    assert dr.num_vertices == V and dr.num_faces == 1532
    att, gt = _batch(pkg, dr, 2, seed=57)
    a, cn = _both(pkg, dr, att, gt)
    assert (cn[:, 1] > 0).all() and (a["face_idx"] >= 0).any()
    assert float(a["grad_vertices"][:, V - 1].abs().max()) > 0      # the last row (an apex of V - 2 faces) is read


# ---- vertices that no face names ------------------------------------------------------------------------------------------------------
def test_unreferenced_vertices(pkg):
    """V = 300, 40 faces (ten strips of four) naming 60 vertices, which lie scattered between 240 rows of +-1e30: the record path never
    loads those, and neither may the order workgroup's result depend on them.  Every output and gradient stays finite."""
    V = 300
    v = np.full((V, 3), 1.0e30, np.float32)
    v[1::7] = -1.0e30
    used = 2 + 5 * np.arange(60)                                   # rows 2, 7, ..., 297
    f = []
    for s in range(10):
        x0, y0 = -0.8 + 0.33 * (s % 5), -0.5 + 0.6 * (s // 5)
        ids = used[6 * s:6 * s + 6]
        for k in range(6):                                         # a zig-zag strip of six vertices: four faces
            v[ids[k]] = (x0 + 0.1 * (k // 2), y0 + 0.3 * (k % 2), 0.05 * s)
        f += [(ids[0], ids[2], ids[1]), (ids[1], ids[2], ids[3]), (ids[2], ids[4], ids[3]), (ids[3], ids[4], ids[5])]
    f = np.array(f, np.int64)
    assert f.shape[0] == 40 and np.unique(f).size == 60 and np.isfinite(v).all()
    dr = _render(pkg, "sphere", 64, mesh=(v, f))
    att, gt = _batch(pkg, dr, 2, seed=55, exact_vertices=True, azimuths=[10.0, 170.0], elevations=[5.0, 20.0], distances=[3.0, 4.0],
                     biases=[[0.0, 0.0], [0.1, -0.1]])
    a, cn = _both(pkg, dr, att, gt)
    _all_finite(a)
    assert (cn[:, 1] > 0).all() and (a["face_idx"] >= 0).any()
    unused = np.setdiff1d(np.arange(V), used)
    assert float(a["grad_vertices"][:, unused].abs().max()) == 0.0 and float(a["grad_vertices"][:, used].abs().max()) > 0


# ---- shared vertices on and behind the camera plane -------------------------------------------------------------------------------------
def _camera_plane_mesh(D):
    """test_gpu_order_in_vertex._border_mesh's last three faces with shared indices: vertex 0 lies ON the camera plane of a camera on the z
    axis at distance D (a division by zero: 0 / 0 in x and y), vertex 1 on it off the axis (a / 0), vertex 2 behind it; each is a corner of
    several faces, one face has all three kinds, and a few ordinary faces in front keep the image covered."""
    v = [(0.0, 0.0, D), (0.3, -0.2, D), (0.1, 0.1, D + 1.0)]
    n = 8
    t = 2.0 * np.pi * np.arange(n) / n
    v += [(0.5 * np.cos(x), 0.5 * np.sin(x), 0.0) for x in t]      # rows 3 .. 10: a ring in front
    v += [(0.0, 0.0, 0.2)]                                         # row 11: the ring's hub
    r = lambda i: 3 + i % n
    f = [(0, r(i), r(i + 1)) for i in range(0, 6, 2)] + [(1, r(i), r(i + 1)) for i in range(1, 6, 2)] + [(2, r(i), r(i + 1)) for i in range(4)]
    f += [(0, 2, r(6)), (1, 2, r(7)), (0, 1, 2)]
    f += [(11, r(i), r(i + 1)) for i in range(n)]
    return np.array(v, np.float32), np.array(f, np.int64)


def test_shared_vertices_on_the_camera_plane(pkg):
    D = 5.0
    v, f = _camera_plane_mesh(D)
    for k in (0, 1, 2):
        assert (f == k).any(axis=1).sum() >= 4
    dr = _render(pkg, "sphere", 64, mesh=(v, f))
    # the camera on the axis (vertices 0 and 1 exactly on its plane), then a little closer and turned by a fraction of a degree
    att, gt = _batch(pkg, dr, 3, seed=59, exact_vertices=True, azimuths=[0.0, 0.0, 0.3], elevations=[0.0, 0.0, 0.2], distances=[D, D - 0.013, D],
                     biases=[[0.0, 0.0]] * 3)
    a, cn = _both(pkg, dr, att, gt)
    assert (cn[:, 1] > 0).all() and (a["face_idx"] >= 0).any()


# ---- the scans over the bins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,ratio,bins", [(256, 1, (32, 32)), (512, 0.25, (64, 16)),
                                          (1024, 1.0 / 16, (128, 8)), (64, 16, (8, 128)), (520, 16.0 / 520, (65, 2)), (16, 520.0 / 16, (2, 65))])
def test_bin_scans(pkg, S, ratio, bins):
    """256x256, B = 1: 32 x 32 bins, the largest square grid the vertex launch sorts (segments of 32 lanes; screens of at most 128 pixels, every
    case above and tests/test_gpu_order_in_vertex.py, scan in segments of 16).  A strip of the same 1 024 tile slots: 64 x 16 bins (a
    wave per line).  Lines longer than a wave keep the scan of a thread per line: 1024x64 (128 x 8 bins) and 64x1024 (8 x 128: a thread per
    column), and the smallest grids one bin past a wave, 520x16 (65 x 2) and 16x520 (2 x 65).  (The step's bits at these shapes from run to
    run: tests/test_gpu_step_reproducible.py.)"""
    dr = _render(pkg, "smpl_uv_642", S, ratio=ratio)
    assert ((dr.image_size + 7) // 8, (dr.render_height + 7) // 8) == bins
    att, gt = _batch(pkg, dr, 1, seed=61, distances=[2.2])
    a, cn = _both(pkg, dr, att, gt)
    assert cn[0, 1] > (16 if min(bins) >= 8 else 0) and (a["face_idx"] >= 0).any()
