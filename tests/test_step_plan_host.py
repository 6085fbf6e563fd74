"""Host side of the step-mode plan tests (tests/test_gpu_step_plan_edges.py): the generated closed templates on both sides of the plan's
switches (F = 4096: one plan workgroup or MM_PLAN_WGS; F = 14 336: counts staged in LDS or re-read), the checker of a face-sweep plan
read back from the workspace, the estimate of an image's texture runs, and mm_render_step_mode on every shape the GPU file uses.
Nothing here needs a GPU; the GPU file imports the helpers from this module."""
import ctypes
import importlib
import os

import numpy as np
import pytest

from conftest import TEMPLATES
from test_gpu_loss_kernels_edges import _icosphere, _write_template

CHUNK_PX = 128                      # MM_CHUNK_PX: pixels of a sweep item at the base chunk size
UV_TILE = 32                        # MM_UV_TILE: edge of a texture tile, in texels
PLAN_SWITCH_FACES = 4096            # more faces than this: MM_PLAN_WGS plan workgroups per image instead of one
SPLIT_FACE = 2376                   # the face of the 4 096-face sphere that the 4 098-face one has in three (visible in the switch tests' images)
PLAN_LDS_FACES = 14336              # more faces than this: the plan re-reads the chunk counts from the face records


# ---------------------------------------------------------------------------------------------------------------------------------
# closed generated templates
# ---------------------------------------------------------------------------------------------------------------------------------
def latlong_sphere(segments=64, stacks=33, split_face=None):
    """Unit sphere cut into `stacks` bands between the poles (on the y axis) and `segments` around: the two polar bands are fans, every other
    band two triangles per segment -- segments * (2 * stacks - 2) faces, wound outwards like _icosphere's.  split_face: that face is replaced
    by the three faces around a new vertex at its centroid (pushed out to the sphere): two faces more, still closed."""
    rings = stacks - 1
    verts = [(0.0, 1.0, 0.0)]
    for i in range(1, stacks):
        th = np.pi * i / stacks
        for j in range(segments):
            ph = 2.0 * np.pi * j / segments
            verts.append((np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)))
    verts.append((0.0, -1.0, 0.0))
    south = len(verts) - 1
    ring = lambda i, j: 1 + i * segments + (j % segments)
    faces = []
    for j in range(segments):
        faces.append((0, ring(0, j + 1), ring(0, j)))
    for i in range(rings - 1):
        for j in range(segments):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            faces += [(a, b, d), (a, d, c)]
    for j in range(segments):
        faces.append((south, ring(rings - 1, j), ring(rings - 1, j + 1)))
    if split_face is not None:
        a, b, c = faces[split_face]
        m = (np.asarray(verts[a]) + np.asarray(verts[b]) + np.asarray(verts[c])) / 3.0
        verts.append(tuple(m / np.sqrt((m * m).sum())))
        n = len(verts) - 1
        faces[split_face:split_face + 1] = [(a, b, n), (b, c, n), (c, a, n)]
    return np.asarray(verts, dtype=np.float32), np.asarray(faces, dtype=np.int64)


GENERATED = {                        # name -> (builder, vertices, faces)
    "icosphere5": (lambda: _icosphere(5), 10242, 20480),
    "latlong4096": (lambda: latlong_sphere(64, 33), 2050, 4096),
    "latlong4098": (lambda: latlong_sphere(64, 33, split_face=SPLIT_FACE), 2051, 4098),
}


def write_generated(directory, name):
    """the generated template `name` as the .npz DiffRender loads, under `directory`; returns its path"""
    v, f = GENERATED[name][0]()
    return _write_template(os.path.join(str(directory), name + ".npz"), v, f)


def template_path(directory, name):
    """a committed template by its name, or a generated one written under `directory`"""
    return write_generated(directory, name) if name in GENERATED else os.path.join(TEMPLATES, name + ".npz")


def edge_uses(faces):
    """how many faces use each undirected edge, and how many times each DIRECTED edge occurs (a consistently wound closed mesh: 2 and 1)"""
    f = np.asarray(faces, dtype=np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    und = np.unique(np.sort(d, 1), axis=0, return_counts=True)[1]
    dire = np.unique(d, axis=0, return_counts=True)[1]
    return und, dire


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(faces)]
    return float((v[:, 0] * np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan of the face sweep (csrc/mm_plan.h), one image
# ---------------------------------------------------------------------------------------------------------------------------------
def check_plan(chunkmap, items, nitems, item_cap, F):
    """The invariants of one image's plan.  chunkmap (F,2) = {first item, items} per face, items (item_cap,2) = {face, chunk of its box},
    nitems (2,) = {items listed, pixels per chunk}.  Raises AssertionError naming the clause; returns (total, k) with chunk = 128 << k.
    Nothing is asserted about the item slots at or beyond total."""
    chunkmap, items, nitems = np.asarray(chunkmap), np.asarray(items), np.asarray(nitems)
    assert chunkmap.shape == (F, 2) and items.shape == (item_cap, 2) and nitems.shape == (2,), (chunkmap.shape, items.shape, nitems.shape)
    total, chunk = int(nitems[0]), int(nitems[1])
    ks = [k for k in range(21) if CHUNK_PX << k == chunk]
    assert ks, "chunk size %d is not 128 << k with 0 <= k <= 20" % chunk
    n = chunkmap[:, 1].astype(np.int64)
    first = chunkmap[:, 0].astype(np.int64)
    assert (n >= 0).all(), "negative item count at face %d" % int(np.argmax(n < 0))
    scan = np.cumsum(n) - n
    bad = np.nonzero(first != scan)[0]
    assert bad.size == 0, "first item of face %d is %d, the exclusive scan of the counts gives %d (%d faces off)" % (
        int(bad[0]), int(first[bad[0]]), int(scan[bad[0]]), bad.size)
    assert total == int(n.sum()), "nitems says %d items, the faces' counts add up to %d" % (total, int(n.sum()))
    assert total <= item_cap, "%d items in a list of %d" % (total, item_cap)
    want_f = np.repeat(np.arange(F, dtype=np.int64), n)
    want_c = np.arange(total, dtype=np.int64) - np.repeat(scan, n)
    got = items[:total].astype(np.int64)
    bad = np.nonzero((got[:, 0] != want_f) | (got[:, 1] != want_c))[0]
    assert bad.size == 0, "item %d is (%d, %d), expected (%d, %d) (%d items off)" % (
        int(bad[0]), int(got[bad[0], 0]), int(got[bad[0], 1]), int(want_f[bad[0]]), int(want_c[bad[0]]), bad.size)
    return total, ks[0]


def make_plan(n, chunk=CHUNK_PX, item_cap=None):
    """a correct plan for the per-face item counts n"""
    n = np.asarray(n, dtype=np.int32)
    F, total = n.size, int(n.sum())
    item_cap = total + 5 if item_cap is None else item_cap
    first = (np.cumsum(n) - n).astype(np.int32)
    items = np.full((item_cap, 2), -7, dtype=np.int32)             # (stale words beyond the list: never looked at)
    items[:total, 0] = np.repeat(np.arange(F, dtype=np.int32), n)
    items[:total, 1] = np.arange(total, dtype=np.int32) - np.repeat(first, n)
    return np.stack([first, n], 1), items, np.asarray([total, chunk], dtype=np.int32), item_cap, F


# ---------------------------------------------------------------------------------------------------------------------------------
# texture runs of step mode (csrc/mm_raster_common.h: step_pixel_pass)
# ---------------------------------------------------------------------------------------------------------------------------------
def expected_runs(face_idx, face_uvs, Ht, Wt, live=None):
    """An ESTIMATE of the runs step mode lists for one image: face_idx (H,W) int (-1: uncovered), face_uvs (F,3,2).  Every wave shades an
    8x8 screen tile and opens, per footprint slot (the footprint's own tile; the tile of its right column, of its lower row, of the opposite
    corner -- each only where it is another tile), one run per distinct 32x32-texel texture tile among the tile's covered pixels.  A pixel's
    uv is taken as the mean of its face's three uvs: exact for the layouts this guards (all three uvs of a face on one point), an estimate
    otherwise.  Pixels whose texture gradient is exactly zero append nothing: live (H,W) bool, if given, marks the pixels that can have one (the
    image term of the loss is weighted by the ground-truth mask: a pixel where that is 0 has none).  Returns the (ceil(H/8), ceil(W/8)) int
    array of runs per screen tile.  It guards the PRECONDITION of the run-list overflow test, never a result."""
    face_idx = np.asarray(face_idx)
    H, W = face_idx.shape
    uv = np.asarray(face_uvs, dtype=np.float32).reshape(-1, 3, 2).mean(1, dtype=np.float32)
    f = np.maximum(face_idx, 0)
    u, v = uv[f, 0], uv[f, 1]
    # bilin_setup (csrc/mm_device.h): grid_sample(align_corners=False, padding_mode='border')
    ix = np.clip(((u * 2 - 1 + 1) * np.float32(Wt) - 1) / 2, 0, Wt - 1)
    iy = np.clip(((-(v * 2 - 1) + 1) * np.float32(Ht) - 1) / 2, 0, Ht - 1)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    x1, y1 = np.where(x0 + 1 < Wt, x0 + 1, x0), np.where(y0 + 1 < Ht, y0 + 1, y0)
    ntx = (Wt + UV_TILE - 1) // UV_TILE
    tx0, ty0, tx1, ty1 = x0 // UV_TILE, y0 // UV_TILE, x1 // UV_TILE, y1 // UV_TILE
    slots = [ty0 * ntx + tx0, np.where(tx1 != tx0, ty0 * ntx + tx1, -1), np.where(ty1 != ty0, ty1 * ntx + tx0, -1),
             np.where((tx1 != tx0) & (ty1 != ty0), ty1 * ntx + tx1, -1)]
    out = np.zeros(((H + 7) // 8, (W + 7) // 8), dtype=np.int64)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            win = (slice(ty * 8, ty * 8 + 8), slice(tx * 8, tx * 8 + 8))
            cov = (face_idx[win] >= 0) if live is None else (face_idx[win] >= 0) & np.asarray(live)[win]
            for s in slots:
                t = s[win][cov]
                out[ty, tx] += np.unique(t[t >= 0]).size
    return out


def corner_uvs(F, Ht, Wt, spread):
    """face_uvs (1,F,3,2) with a face's three uvs on ONE corner shared by four texture tiles, at its texel centre (texel coordinates
    (32 i - 0.5, 32 j - 0.5)): spread False -- every face on corner (1, 1), the layout of the record-pool overflow tests; spread True --
    face f on interior corner number f mod n of the n = (ntx - 1)(nty - 1) there are."""
    ntx, nty = (Wt + UV_TILE - 1) // UV_TILE, (Ht + UV_TILE - 1) // UV_TILE
    nx, ny = ntx - 1, nty - 1
    assert nx >= 1 and ny >= 1
    k = np.arange(F) % (nx * ny) if spread else np.zeros(F, dtype=np.int64)
    i, j = 1 + k % nx, 1 + k // nx
    uv = np.empty((1, F, 3, 2), dtype=np.float32)
    uv[0, :, :, 0] = (np.float32(UV_TILE) * i / np.float32(Wt))[:, None]
    uv[0, :, :, 1] = (1.0 - np.float32(UV_TILE) * j / np.float32(Ht))[:, None]
    return uv


def box_pixels(fvi, boxlen, H, W):
    """Pixels of every face's box inflated by the soft-mask margin and clipped to the image, (B,F) int64, from the oracle's image-plane
    corners fvi (B,F,3,2) in [-1, 1]: the pixels whose centres 2 (i + 0.5) / n - 1 lie in [min - boxlen, max + boxlen], with the 0.02 px of
    slack the vertex stage allows itself (csrc/mm_device.h: pixel_range).  A host count to DECIDE a case's numbers by, never an expectation."""
    fvi = np.asarray(fvi, dtype=np.float64)
    lo, hi = fvi.min(2) - boxlen, fvi.max(2) + boxlen
    n = []
    for ax, size in ((0, W), (1, H)):
        i0 = np.ceil((lo[..., ax] + 1) * size / 2 - 0.5 - 0.02)
        i1 = np.floor((hi[..., ax] + 1) * size / 2 - 0.5 + 0.02)
        n.append(np.clip(np.minimum(i1, size - 1) - np.maximum(i0, 0) + 1, 0, None))
    return (n[0] * n[1]).astype(np.int64)


def predicted_doublings(px, item_cap):
    """k per image: the chunk size 128 << k at which the boxes of px (B,F) fit item_cap items"""
    out = []
    for row in np.asarray(px):
        k = 0
        while int(((row + (CHUNK_PX << k) - 1) // (CHUNK_PX << k)).sum()) > item_cap:
            k += 1
        out.append(k)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_step_plan_edges.py: (template, B, S, H) -- all with 8-pixel screen bins
# ---------------------------------------------------------------------------------------------------------------------------------
STEP_SHAPES = [("smpl_uv", 2, 64, 64), ("smpl_uv", 3, 72, 56), ("sphere2", 3, 40, 40), ("latlong4096", 3, 48, 48), ("latlong4098", 3, 48, 48),
               ("icosphere5", 2, 64, 64), ("icosphere5", 2, 72, 56), ("smpl_uv", 3, 64, 64), ("icosphere5", 3, 64, 64), ("sphere", 3, 32, 32)]


def _sizes(name):
    if name in GENERATED:
        return GENERATED[name][1], GENERATED[name][2]
    z = np.load(os.path.join(TEMPLATES, name + ".npz"))
    return int(z["vertices"].shape[0]), int(z["faces"].shape[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen_dir(tmp_path_factory):                                     # (tests/test_gpu_step_plan_edges.py imports it)
    return tmp_path_factory.mktemp("step_plan_templates")


@pytest.mark.parametrize("name", sorted(GENERATED))
def test_generated_templates_are_closed_and_load(pkg, gen_dir, name):
    """Both sides of F = 4096 are the lat-long sphere (64 segments, 33 stacks, polar fans) and the same sphere with face SPLIT_FACE split in three;
    F > 14 336 is the subdivision-5 icosphere.  Closed: every edge in two faces, once in each direction; wound outwards like the icosphere of
    tests/test_gpu_loss_kernels_edges.py.  DiffRender's tables (flip_pairing, edge_tables, the vertex-corner table) take all three."""
    _, V, F = GENERATED[name]
    v, f = GENERATED[name][0]()
    assert v.shape == (V, 3) and f.shape == (F, 3) and v.dtype == np.float32
    assert f.min() == 0 and f.max() == V - 1 and np.unique(f).size == V
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 2] != f[:, 0]).all()
    und, dire = edge_uses(f)
    assert und.size == 3 * F // 2 and (und == 2).all() and (dire == 1).all()
    assert V - und.size + F == 2                                   # a sphere
    assert signed_volume(v, f) > 4.0 and signed_volume(*_icosphere(1)) > 0       # (unit sphere: 4.19) the same winding as _icosphere
    dr = pkg.DiffRender(write_generated(gen_dir, name), 32, emit_imnormal=True)
    assert (dr.num_vertices, dr.num_faces) == (V, F) and dr.edges.shape[0] == 3 * F // 2
    assert tuple(dr.face_uvs.shape) == (1, F, 3, 2) and tuple(dr.flip_index.shape) == (V,)
    assert (F > PLAN_SWITCH_FACES) == (name != "latlong4096") and (F > PLAN_LDS_FACES) == (name == "icosphere5")


def test_the_split_sphere_is_the_smallest_closed_mesh_above_the_switch():
    """A closed triangle mesh has an even face count (3F = 2E), so 4 098 is the first above 4 096; and it is the 4 096-face sphere but for
    one face: the two render nearly the same image."""
    v0, f0 = GENERATED["latlong4096"][0]()
    v1, f1 = GENERATED["latlong4098"][0]()
    assert f1.shape[0] == PLAN_SWITCH_FACES + 2 and f0.shape[0] == PLAN_SWITCH_FACES
    assert np.array_equal(v0, v1[:-1]) and np.array_equal(f0[:SPLIT_FACE], f1[:SPLIT_FACE]) and np.array_equal(f0[SPLIT_FACE + 1:], f1[SPLIT_FACE + 3:])
    assert abs(float(np.linalg.norm(v1[-1])) - 1.0) < 1e-6


def test_check_plan_accepts_good_plans():
    rng = np.random.default_rng(0)
    for F, chunk in ((1, 128), (7, 128), (300, 256), (5000, 128 << 20)):
        n = rng.integers(0, 4, size=F)
        total, k = check_plan(*make_plan(n, chunk=chunk))
        assert total == int(n.sum()) and 128 << k == chunk
    check_plan(*make_plan(np.zeros(9, dtype=np.int32)))                       # nothing to sweep
    check_plan(*make_plan([2, 0, 3], item_cap=5))                             # a list that is exactly full


def _broken_plans():
    """(label, plan) of plans wrong in one clause each"""
    n = np.asarray([1, 2, 0, 3, 1, 0, 2, 1], dtype=np.int32)

    def plan(**kw):
        cm, it, ni, cap, F = make_plan(n, **kw)
        return [cm.copy(), it.copy(), ni.copy(), cap, F]
    out = []
    for chunk in (0, 64, 192, 129, 128 << 21, -128):
        p = plan(); p[2][1] = chunk
        out.append(("chunk %d" % chunk, p))
    p = plan(); p[0][3, 0] += 1
    out.append(("one face's first item off by one", p))
    p = plan(); p[0][4:, 0] -= int(n[:4].sum())
    out.append(("the second half numbered from zero again: the carry between plan workgroups is missing", p))
    p = plan(); p[0][2:, 0] += 1
    out.append(("a gap in the numbering", p))
    p = plan(); p[0][3, 1] = -1
    out.append(("a negative count", p))
    p = plan(); p[2][0] += 1
    out.append(("nitems above the sum", p))
    p = plan(); p[2][0] -= 1
    out.append(("nitems below the sum", p))
    p = plan(item_cap=int(n.sum())); p[3] -= 1; p[1] = p[1][:-1]
    out.append(("more items than the list holds", p))
    p = plan(); p[1][4, 0] = 2
    out.append(("an item of the wrong face", p))
    p = plan(); p[1][4, 1] = 0; p[1][5, 1] = 1
    out.append(("a face's chunks out of order", p))
    p = plan(); p[1][int(n.sum()) - 1] = (-7, -7)
    out.append(("the last item never written", p))
    # what the missing carry leaves behind when the ITEMS are written with it missing too: the quarters' items on top of each other
    p = plan()
    half = int(n[:4].sum())
    p[0][4:, 0] -= half
    tail = p[1][half:int(n.sum())].copy()
    p[1][:tail.shape[0]] = tail
    out.append(("overlapping quarters, items included", p))
    p = plan(); p[0] = p[0][:-1]
    out.append(("a chunkmap of the wrong length", p))
    return out


@pytest.mark.parametrize("label,plan", _broken_plans(), ids=[l for l, _ in _broken_plans()])
def test_check_plan_rejects_a_plan_broken_in_one_clause(label, plan):
    with pytest.raises(AssertionError):
        check_plan(*plan)


def test_check_plan_ignores_the_slots_beyond_the_list():
    cm, it, ni, cap, F = make_plan([2, 1, 4], item_cap=40)
    it[7:] = np.random.default_rng(1).integers(-5, 5, size=it[7:].shape)
    check_plan(cm, it, ni, cap, F)


def test_expected_runs_of_the_corner_layouts():
    """Every face on the one corner (the record-pool overflow tests' layout): four runs per screen tile with a covered pixel, none elsewhere,
    whatever the faces.  Faces spread over the 49 interior corners of a 256x256 texture: four runs per distinct corner in the tile."""
    rng = np.random.default_rng(2)
    F, H, W = 1280, 24, 40
    fidx = rng.integers(-1, F, size=(H, W)).astype(np.int32)
    fidx[8:16, 8:24] = -1                                                     # two empty tiles
    fidx[16:24, 32:40] = -1; fidx[17, 33] = 5                                 # one pixel in a tile
    one = expected_runs(fidx, corner_uvs(F, 64, 64, False)[0], 64, 64)
    assert one.shape == (3, 5) and one.max() <= 4
    assert one[1, 1] == 0 and one[1, 2] == 0 and one[2, 4] == 4 and (np.delete(one.ravel(), [6, 7]) == 4).all()
    many = expected_runs(fidx, corner_uvs(F, 256, 256, True)[0], 256, 256)
    for ty in range(3):
        for tx in range(5):
            t = fidx[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
            assert many[ty, tx] == 4 * np.unique(t[t >= 0] % 49).size
    assert many.max() > 100
    live = np.zeros((H, W), dtype=bool); live[:8] = True                     # only the first row of tiles can have a texture gradient
    assert np.array_equal(expected_runs(fidx, corner_uvs(F, 256, 256, True)[0], 256, 256, live=live), many * np.asarray([[1], [0], [0]]))
    # a footprint inside one tile is one run; one that straddles only a vertical border, two
    uv = np.empty((2, 3, 2), dtype=np.float32)
    uv[0] = (10.0 / 64, 1.0 - 10.0 / 64); uv[1] = (32.0 / 64, 1.0 - 10.0 / 64)
    f2 = np.full((8, 8), -1, dtype=np.int32); f2[0, 0] = 0
    assert expected_runs(f2, uv, 64, 64).tolist() == [[1]]
    f2[0, 1] = 1
    assert expected_runs(f2, uv, 64, 64).tolist() == [[2]]                    # slot 0: tile 0 for both; slot 1: tile 1 for the second


def test_corner_uvs_sit_on_texel_centres_between_four_tiles():
    uv = corner_uvs(200, 256, 256, True)[0, :, 0]
    x = uv[:, 0] * 256 - 0.5; y = (1 - uv[:, 1]) * 256 - 0.5
    assert np.array_equal(x % 32, np.full(200, 31.5)) and np.array_equal(y % 32, np.full(200, 31.5))
    assert np.unique(np.stack([x, y], 1), axis=0).shape[0] == 49 and x.min() == 31.5 and x.max() == 223.5
    one = corner_uvs(5, 64, 64, False)[0]
    assert np.array_equal(one, np.full((5, 3, 2), 0.5, dtype=np.float32))      # texel coordinates (31.5, 31.5) of a 64x64 texture


def _mode(N, name, B, S, H, **kw):
    V, F = _sizes(name)
    d = N.MMRenderDesc()
    d.B, d.H, d.W, d.V, d.F, d.Ht, d.Wt, d.knum, d.no_mask = B, H, S, V, F, 2 * H, S, 30, 1
    g = N.MMRenderGrads()
    bg, gt = ctypes.c_float(), (ctypes.c_float * 4)()
    g.grad_bg = ctypes.addressof(bg)
    d.step_grads, d.fused_gt = ctypes.addressof(g), ctypes.addressof(gt)
    for k, v in kw.items():
        setattr(d, k, v)
    return N.lib().mm_render_step_mode(ctypes.byref(d))


@pytest.mark.parametrize("name,B,S,H", STEP_SHAPES)
def test_step_mode_is_taken_at_every_shape_of_the_gpu_file(pkg, name, B, S, H):
    N = importlib.import_module("3d-magic-mirror_amd._native")
    assert _mode(N, name, B, S, H) == 1
    assert _mode(N, name, B, S, H, no_mask=0) == 1
    assert _mode(N, name, B, S, H, knum=80, boxlen=0.3, sigmainv=60.0) == 1
    assert _mode(N, name, B, S, H, step_grads=None) == 0


def test_step_mode_is_refused_where_screen_bins_are_sixteen_pixels(pkg):
    """smpl_uv (13 776 faces): 8-pixel bins up to 72x72, 16-pixel bins at 80x80 -- the compacting walk, which step mode does not cover."""
    N = importlib.import_module("3d-magic-mirror_amd._native")
    assert _mode(N, "smpl_uv", 2, 72, 72) == 1
    assert _mode(N, "smpl_uv", 2, 80, 80) == 0
    assert _mode(N, "sphere2", 2, 128, 128) == 1


def test_box_pixels_and_predicted_doublings():
    fvi = np.zeros((1, 3, 3, 2))
    fvi[0, 0] = [(-0.5, -0.5), (0.0, -0.5), (-0.5, 0.0)]            # centres at -0.4375 ... -0.0625 of a 16-pixel axis: pixels 4..7
    fvi[0, 1] = [(0.9, 0.9), (0.95, 0.9), (0.9, 0.95)]               # one centre inside (0.9375); with a margin, clipped by the border
    fvi[0, 2] = [(3.0, 3.0), (3.5, 3.0), (3.0, 3.5)]                 # off the image
    assert box_pixels(fvi, 0.0, 16, 16).tolist() == [[16, 1, 0]]
    assert box_pixels(fvi, 0.125, 16, 16).tolist() == [[36, 4, 0]]
    assert box_pixels(fvi, 0.125, 8, 16).tolist() == [[24, 2, 0]]     # (a centre exactly on the closed border counts)
    assert predicted_doublings([[128, 129, 0], [1000, 1000, 1000], [128, 128, 128]], 3) == [0, 3, 0]
