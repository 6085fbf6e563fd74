"""Step mode (MMRenderDesc.step_grads) where its code branches and no other test goes: four plan workgroups per image (F > 4096) with and
without spare workgroups in front of the walk, the switch itself (4 096 against 4 098 faces), the unstaged plan (F > 14 336: the first run
of that branch in either home of the plan), chunk doubling in both, the run list's own capacity, and the soft mask away from its defaults.

Every case is built as tests/test_gpu_fused_step.py::_step builds it (the same draws in the same order; the extra knobs are listed at
_Case) and runs once in step mode and once with the field unset.  Three checks per case:
  (a) the two runs are equal BIT FOR BIT (image, face_idx, normals, loss, all gradients: _same of tests/test_gpu_fused_step.py);
  (b) the plan of the face sweep, read back from the workspace (mm_debug_workspace_layout), passes check_plan (tests/test_step_plan_host.py)
      for every image and is identical between the two runs -- at 8-pixel screen bins neither path has face flags;
  (c) step mode against the CPU oracle at the project's bars: face_idx equal, image within 1e-4, loss within 2e-5, every gradient within
      1e-4 of its own maximum (tests/parity_bar.py; the float64 oracle judges a miss, a `cond` verdict is printed with its two distances and
      no case may be all `cond`).  The two paths share csrc/mm_pixel_pass.h and csrc/mm_plan.h: only (c) sees a fault in the shared text.
Beyond check_plan, (b) holds the plan to the oracle's face_idx: a face that owns pixels has items, and its items' pixels are no fewer than
the pixels it owns (they lie inside its box).  Each precondition (step mode taken, F on its side of a switch, a doubled chunk somewhere,
runs beyond the list with records below the array) is asserted before any result is looked at."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from parity_bar import grad_close, rel_errors
from test_gpu_fused_step import LEAVES, _arrays, _bits, _same, _step
from test_gpu_parity import _close
from test_step_plan_host import gen_dir  # noqa: F401  (the fixture: the directory the generated templates are written to)
from test_step_plan_host import (CHUNK_PX, GENERATED, PLAN_LDS_FACES, PLAN_SWITCH_FACES, SPLIT_FACE, box_pixels, check_plan, corner_uvs,
                                 expected_runs, predicted_doublings, template_path)

pytestmark = pytest.mark.gpu


class _Case:
    """The inputs of _step (tests/test_gpu_fused_step.py), drawn in its order, kept on the host for the oracle; .step(step_mode) is the
    RenderLossStep.  Beyond _step's arguments: name may be a generated template (tests/test_step_plan_host.py: GENERATED); soft = (knum,
    boxlen, sigmainv); uvs = "one" (_step's uv_corner) or "spread" (face f on interior tile corner f mod n of the texture); extra =
    DiffRender.extra_texture_records_per_pixel; smooth = s: vertices = template + s * the batch's delta (the default batch moves every vertex by
    0.05 sigma, which crumples a mesh whose edges are shorter than that into faces of several pixels); draws_of = another generated template
    whose vertex count the draws are made for: the first that many vertices get exactly that template's batch and every further vertex sits at
    the mean of its neighbours, so that two meshes which differ in one split face render the same surface from the same cameras.
    _step cannot be called itself (it keeps nothing on the host for the oracle and loads committed templates only), so its draws are
    written out again here: test_case_builder_draws_what_step_draws holds the two builders together, bit for bit."""

    def __init__(self, pkg, gen_dir, name, B, S, ratio=1, seed=0, no_mask=True, tex=None, dist=None, soft_gt=False, soft=None, uvs=None,
                 extra=0.0, smooth=None, draws_of=None):
        self.pkg, self.B, self.no_mask, self.soft = pkg, B, no_mask, soft
        dr = pkg.DiffRender(template_path(gen_dir, name), S, ratio=ratio, emit_imnormal=True)
        if soft is not None:
            dr.knum, dr.boxlen, dr.sigmainv = soft
        dr.extra_texture_records_per_pixel = extra
        H, W = dr.render_height, dr.image_size
        V0 = GENERATED[draws_of][1] if draws_of else dr.num_vertices
        att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init[:V0], B, H, W, seed=seed)
        g = torch.Generator(device="cpu").manual_seed(1000 + seed)
        if tex is not None:
            att["textures"] = torch.rand(B, 3, tex[0], tex[1], generator=g)
        if dist is not None:
            att["distances"] = torch.full((B,), float(dist)) if np.isscalar(dist) else torch.tensor(dist, dtype=torch.float32)
        if soft_gt:
            gt = gt.clone()
            gt[:, 3] = torch.rand(B, H, W, generator=g)
        if smooth is not None:
            att["vertices"] = dr.vertices_init[None] + float(smooth) * att["delta_vertices"]
        if V0 < dr.num_vertices:
            faces = dr.faces.numpy()
            more = []
            for n in range(V0, dr.num_vertices):
                ring = np.unique(faces[(faces == n).any(1)])
                more.append(att["vertices"][:, torch.from_numpy(ring[ring < V0])].mean(1, keepdim=True))
            att["vertices"] = torch.cat([att["vertices"]] + more, 1)
        if uvs is not None:
            Ht, Wt = att["textures"].shape[2:]
            dr.face_uvs = torch.from_numpy(corner_uvs(dr.num_faces, Ht, Wt, uvs == "spread"))
        assert att["vertices"].shape == (B, dr.num_vertices, 3)
        self.dr, self.att, self.gt, self.H, self.W = dr, att, gt, H, W
        self.inp = {k: v.numpy() for k, v in att.items() if torch.is_tensor(v)}
        self.inp["faces"] = dr.faces.numpy().astype(np.int32)
        self.inp["face_uvs"] = dr.face_uvs.numpy()[0]
        self.proj = dr.cam_proj.numpy().reshape(3)
        self.kw = {} if soft is None else dict(knum=soft[0], boxlen=soft[1], sigmainv=soft[2])

    def step(self, step_mode):
        stepmod = importlib.import_module("3d-magic-mirror_amd.step")
        dev = torch.device("cuda:0")
        att = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in self.att.items()}
        return stepmod.RenderLossStep(self.dr, att, self.gt.to(dev), no_mask=self.no_mask, emit_imnormal=True, fused=True, step_mode=step_mode)

    def pair(self):
        """(step mode, field unset), both run once; step mode must have been taken"""
        new, old = self.step(True), self.step(False)
        assert new.step_mode_taken() and not old.step_mode_taken()
        new.run(); old.run()
        torch.cuda.synchronize()
        return new, old

    def oracle_forward(self, oracle):
        return oracle.render_forward(self.inp, self.H, self.W, self.no_mask, self.proj, **self.kw)

    def oracle_step(self, oracle, dtype=np.float32):
        return oracle.step(self.inp, self.gt.numpy(), self.H, self.W, self.no_mask, self.proj, image_weight=self.dr.image_weight, dtype=dtype, **self.kw)


def _plan(st):
    """the plan arrays of a step's workspace: chunkmap (B,F,2), items (B,item_cap,2), nitems (B,2), item_cap"""
    N = importlib.import_module("3d-magic-mirror_amd._native")
    out = (ctypes.c_size_t * 16)()
    assert N.lib().mm_debug_workspace_layout(ctypes.byref(st.d), out) == 0
    torch.cuda.synchronize()
    B, F, cap = st.B, st.dr.num_faces, int(out[4])
    assert cap == F + (16 * st.H * st.W + CHUNK_PX - 1) // CHUNK_PX          # the documented capacity (csrc/mm_device.h)
    grab = lambda off, n: st.ws[off:off + n * 8].view(torch.int32).reshape(n, 2).cpu().numpy()
    return grab(out[0], B * F).reshape(B, F, 2), grab(out[1], B * cap).reshape(B, cap, 2), grab(out[2], B), cap


def _check_plans(new, old, face_idx_ref, label):
    """(b): returns the doublings k per image"""
    cm, it, ni, cap = _plan(new)
    cm2, it2, ni2, cap2 = _plan(old)
    F, ks = new.dr.num_faces, []
    for b in range(new.B):
        for tag, (c, i, n) in (("step mode", (cm[b], it[b], ni[b])), ("two-pass", (cm2[b], it2[b], ni2[b]))):
            try:
                total, k = check_plan(c, i, n, cap, F)
            except AssertionError as e:
                raise AssertionError("%s, image %d, %s plan: %s" % (label, b, tag, e))
            owned = np.bincount(face_idx_ref[b][face_idx_ref[b] >= 0], minlength=F)
            short = np.nonzero(c[:, 1].astype(np.int64) * (CHUNK_PX << k) < owned)[0]
            assert short.size == 0, "%s, image %d, %s plan: face %d owns %d pixels and has %d items of %d pixels (%d such faces)" % (
                label, b, tag, int(short[0]), int(owned[short[0]]), int(c[short[0], 1]), CHUNK_PX << k, short.size)
        ks.append(k)
        assert np.array_equal(ni[b], ni2[b]), "%s, image %d: nitems %s in step mode, %s in the two-pass step" % (label, b, ni[b], ni2[b])
        assert np.array_equal(cm[b], cm2[b]), "%s, image %d: the chunkmaps of the two paths differ" % (label, b)
        assert np.array_equal(it[b][:total], it2[b][:total]), "%s, image %d: the item lists of the two paths differ" % (label, b)
    print("%s: items per image %s of %d, chunk px %s" % (label, ni[:, 0].tolist(), cap, ni[:, 1].tolist()))
    return ks


def _check_oracle(case, oracle, st, got, label):
    """(c) for the step st (its outputs in got): returns the verdicts per gradient"""
    rgba_o, fidx_o, fn_o, imn_o = case.oracle_forward(oracle)
    fidx = got["face_idx"].cpu().numpy()
    assert (fidx == fidx_o).all(), "%s: face_idx mismatches: %d" % (label, int((fidx != fidx_o).sum()))
    assert (fidx_o >= 0).any(axis=(1, 2)).all() and (fidx_o < 0).any()
    _close(got["rgba"].cpu().numpy(), rgba_o)
    loss_o, g_o = case.oracle_step(oracle)
    assert abs(float(got["loss"]) - loss_o) < 2e-5, (label, float(got["loss"]), loss_o)
    g64 = {}

    def ref64(k):
        if not g64:
            g64.update(case.oracle_step(oracle, dtype=np.float64)[1])
        return g64[k]
    verdicts = {}
    for k in LEAVES:
        if k == "bg" and not case.no_mask:
            assert "grad_bg" not in got
            continue
        assert float(np.abs(g_o[k]).max()) > 0, (label, k)
        verdicts[k] = grad_close(got["grad_" + k], g_o[k], rtol=1e-4, what="%s, %s" % (label, k), ref64=lambda k=k: ref64(k))
        if verdicts[k] == "cond":
            print("%s: COND %s: to the float64 oracle, HIP %.3e, fp32 oracle %.3e (of the gradient's maximum)" % (
                label, k, rel_errors(got["grad_" + k], ref64(k))[0], rel_errors(g_o[k], ref64(k))[0]))
    print("%s: verdicts %s" % (label, verdicts))
    assert any(v == "ok" for v in verdicts.values()), (label, verdicts)
    return fidx_o, verdicts


def _check(case, oracle, label):
    """(a), (b), (c) of one case; returns (step-mode step, two-pass step, doublings per image)"""
    new, old = case.pair()
    assert new.dropped_records() == [0] * case.B and old.dropped_records() == [0] * case.B
    a = _arrays(new)
    fidx_o, _ = _check_oracle(case, oracle, new, a, label)
    ks = _check_plans(new, old, fidx_o, label)
    _same(a, _arrays(old))
    return new, old, ks


def _plan_workgroups(F, B):
    """(plan workgroups per image, workgroups in front of the walk, how many of them have nothing to do), as csrc/mm_raster.hip sizes its
    grid.  It pins NOTHING in the kernel -- the grid cannot be observed from here: it only says, next to the case, which layout of the
    grid's front the case's F and B were chosen for, and fails if a case's numbers are changed without its docstring."""
    wgs = 4 if F > PLAN_SWITCH_FACES else 1
    first = (wgs * B + 7) & ~7
    return wgs, first, first - wgs * B


# ---- 0. the builder of the cases against the builder it restates ---------------------------------------------------------------------
def test_case_builder_draws_what_step_draws(pkg, gen_dir):
    """_Case draws its inputs in the order of tests/test_gpu_fused_step.py::_step (the batch, then from one generator: the texture, the soft
    ground-truth mask; distances and the one-corner uvs are set, not drawn).  The same arguments to both give the same step: every output and
    gradient equal bit for bit, in step mode, on a committed template.  Should either builder change its draws, this fails first."""
    kw = dict(ratio=0.6, seed=23, no_mask=False, tex=(64, 32), dist=[2.0, 2.6, 3.3], soft_gt=True)
    case = _Case(pkg, gen_dir, "sphere", 3, 40, **kw)
    mine, theirs = case.step(True), _step(pkg, "sphere", 3, 40, step_mode=True, **kw)
    assert mine.step_mode_taken() and theirs.step_mode_taken() and (mine.H, mine.W) == (theirs.H, theirs.W) == (24, 40)
    mine.run(); theirs.run()
    a = _arrays(mine)
    _same(a, _arrays(theirs))
    assert bool(torch.isfinite(a["grad_textures"]).all()) and float(a["grad_textures"].abs().max()) > 0
    assert torch.equal(_bits(case.gt), _bits(theirs.gt.cpu()))
    # the one-corner layout: _step's uv_corner against corner_uvs
    one = _Case(pkg, gen_dir, "sphere", 2, 32, seed=23, tex=(64, 64), uvs="one")
    ref = _step(pkg, "sphere", 2, 32, seed=23, tex=(64, 64), uv_corner=True)
    assert torch.equal(_bits(one.dr.face_uvs), _bits(ref.dr.face_uvs))


# ---- 1. four plan workgroups per image, counts staged in LDS ------------------------------------------------------------------------
@pytest.mark.parametrize("no_mask", [True, False])
@pytest.mark.parametrize("B,S,H,first,spare", [(2, 64, 64, 8, 0), (3, 72, 56, 16, 4)])
def test_four_plan_workgroups_staged(pkg, oracle, gen_dir, B, S, H, first, spare, no_mask):
    """smpl_uv, 13 776 faces: every image's plan is written by four workgroups, each a quarter, numbered behind the quarters in front
    (the carry).  B = 2: the eight plan workgroups are all of the grid's front; B = 3 at 56x72: twelve of sixteen, four leave at once, and
    the image's last row of blocks is ragged."""
    case = _Case(pkg, gen_dir, "smpl_uv", B, S, ratio=H / S, seed=61 + B, no_mask=no_mask)
    F = case.dr.num_faces
    assert (case.H, case.W) == (H, S) and PLAN_SWITCH_FACES < F <= PLAN_LDS_FACES and _plan_workgroups(F, B) == (4, first, spare)
    _check(case, oracle, "smpl_uv B=%d %dx%d no_mask=%s" % (B, H, S, no_mask))


def test_four_plan_workgroups_soft_ground_truth(pkg, oracle, gen_dir):
    """sphere2, 5 120 faces (five faces per plan thread, the last threads' ranges empty), with a ground-truth mask all over [0, 1]"""
    case = _Case(pkg, gen_dir, "sphere2", 3, 40, seed=64, soft_gt=True)
    assert PLAN_SWITCH_FACES < case.dr.num_faces <= PLAN_LDS_FACES
    _check(case, oracle, "sphere2 B=3 40x40 soft gt")


# ---- 2. the switch ------------------------------------------------------------------------------------------------------------------
def _switch_case(pkg, gen_dir, name):
    return _Case(pkg, gen_dir, name, 3, 48, seed=65, draws_of="latlong4096")


@pytest.mark.parametrize("name", ["latlong4096", "latlong4098"])
def test_the_switch_between_one_and_four_plan_workgroups(pkg, oracle, gen_dir, name):
    """The 4 096-face lat-long sphere (one plan workgroup, sixteen faces per thread) and the same sphere with face SPLIT_FACE split in three (four
    workgroups, five faces per thread, threads 820 ... 1023 with empty ranges): the same batch -- the new vertex sits in its face's plane --
    so the two render the same surface from the same cameras.  Both plans are complete: base chunk size, every face that owns a pixel
    listed, the last face's items end the list."""
    case = _switch_case(pkg, gen_dir, name)
    F = case.dr.num_faces
    assert (F > PLAN_SWITCH_FACES) == (name == "latlong4098") and _plan_workgroups(F, 3)[0] == (4 if name == "latlong4098" else 1)
    new, old, ks = _check(case, oracle, name + " B=3 48x48")
    cm, it, ni, cap = _plan(new)
    assert ks == [0, 0, 0] and (ni[:, 1] == CHUNK_PX).all()
    for b in range(3):
        assert int(cm[b, -1, 0]) + int(cm[b, -1, 1]) == int(ni[b, 0]) and int(ni[b, 0]) >= int((cm[b, :, 1] > 0).sum()) > 0


def test_the_two_sides_of_the_switch_plan_the_shared_faces_alike(pkg, gen_dir):
    """Every face but the split one has the same three vertices in both meshes, bit for bit, hence the same box and the same item count:
    the plans of the two sides of the switch differ only where the meshes do."""
    plans = {}
    for name in ("latlong4096", "latlong4098"):
        case = _switch_case(pkg, gen_dir, name)
        st = case.step(True)
        assert st.step_mode_taken()
        st.run()
        plans[name] = (_plan(st)[0], case)
    (cm0, c0), (cm1, c1) = plans["latlong4096"], plans["latlong4098"]
    assert np.array_equal(c0.inp["vertices"], c1.inp["vertices"][:, :-1]) and np.array_equal(c0.inp["azimuths"], c1.inp["azimuths"])
    s = SPLIT_FACE
    assert np.array_equal(cm0[:, :s, 1], cm1[:, :s, 1]) and np.array_equal(cm0[:, s + 1:, 1], cm1[:, s + 3:, 1])
    assert np.array_equal(cm0[:, :s + 1, 0], cm1[:, :s + 1, 0]) and (cm1[:, s:s + 3, 1] <= cm0[:, s:s + 1, 1]).all()
    assert int(cm0[:, :, 1].sum()) > 0


# ---- 3. the unstaged plan -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,H", [(64, 64), (72, 56)])
def test_unstaged_plan(pkg, oracle, gen_dir, S, H):
    """The 20 480-face icosphere: more faces than the plan's LDS holds counts for, so every pass re-reads the face records."""
    case = _Case(pkg, gen_dir, "icosphere5", 2, S, ratio=H / S, seed=66)
    assert case.dr.num_faces > PLAN_LDS_FACES and (case.H, case.W) == (H, S)
    _check(case, oracle, "icosphere5 B=2 %dx%d" % (H, S))


# ---- 4. chunk doubling --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,boxlen,want", [("smpl_uv", 0.12, "mixed"), ("icosphere5", 0.12, "mixed"), ("smpl_uv", 0.3, "deep")])
def test_chunk_doubling(pkg, oracle, gen_dir, name, boxlen, want):
    """knum 80, sigmainv 60 and a wide box at 64x64, cameras at 1.9, 2.6 and 9.0.  With boxlen 0.3 (the triple of
    test_soft_mask_truncation_and_margins_match_oracle) every face's box has ~400 pixels at every one of these distances: all three images
    double, twice or more ("deep"), and none stays at 128.  The host count of inflated box pixels (box_pixels over oracle.prepare_vertices)
    puts the mix at boxlen 0.12: base items 16 192 / 15 896 / 13 776 of 14 288 for smpl_uv (two images double once, the far one does not),
    19 583 / 24 167 / 20 480 of 20 992 for the icosphere (the middle one doubles; there chunks() divides instead of shifting)."""
    case = _Case(pkg, gen_dir, name, 3, 64, seed=41, soft=(80, boxlen, 60.0), dist=[1.9, 2.6, 9.0])
    F = case.dr.num_faces
    assert (F > PLAN_LDS_FACES) == (name == "icosphere5") and F > PLAN_SWITCH_FACES
    fvi = oracle.prepare_vertices(case.inp["vertices"], case.inp["faces"], oracle.camera(
        case.inp["distances"], case.inp["elevations"], case.inp["azimuths"], case.inp["biases"]), case.proj)[1]
    print("host count: doublings", predicted_doublings(box_pixels(fvi, boxlen, 64, 64), F + 16 * 64 * 64 // CHUNK_PX))
    new, old, ks = _check(case, oracle, "%s boxlen %.2f" % (name, boxlen))
    if want == "mixed":
        assert max(ks) >= 1 and min(ks) == 0, ks              # a chunk of 256 or more in one image, 128 in another
    else:
        assert min(ks) >= 1 and max(ks) >= 2, ks


# ---- 5. the run list's own capacity -------------------------------------------------------------------------------------------------
def _runs_case(pkg, gen_dir, name, uvs, **kw):
    """(a ground-truth mask without zeros: the image term is weighted by it, and a covered pixel where it is 0 appends no record)"""
    return _Case(pkg, gen_dir, name, 2, 64, seed=51, tex=(256, 256), uvs=uvs, extra=3.0, soft_gt=True, **kw)


def _run_numbers(case, st, fidx_o):
    """(estimated runs per image, runcap, records needed per image, trcap) -- trcap from the workspace the step really has"""
    N = importlib.import_module("3d-magic-mirror_amd._native")
    out = (ctypes.c_size_t * 4)()
    assert N.lib().mm_debug_step_layout(ctypes.byref(st.d), out) == 0
    runcap = int(out[3])
    live = case.gt[:, 3].numpy() != 0
    est = [int(expected_runs(fidx_o[b], case.inp["face_uvs"], 256, 256, live=live[b]).sum()) for b in range(case.B)]
    need = [4 * int(((fidx_o[b] >= 0) & live[b]).sum()) for b in range(case.B)]
    trcap = runcap + int(np.ceil(3.0 * case.H * case.W))                     # the minimum array + the extra records asked for
    assert runcap == (case.H * case.W * 9 // 8 + 255) // 256 * 256            # the list stays at the minimum (csrc/mm_device.h)
    return est, runcap, need, trcap


def test_run_list_overflow_is_loud(pkg, oracle, gen_dir):
    """Run list full, record array not.  Texture 256x256 (49 interior tile corners), face f's uvs on corner f mod 49: four records per covered
    pixel, and in every 8x8 screen tile four runs per distinct corner.  extra_texture_records_per_pixel = 3: the array holds 4 1/8 H W records,
    the list stays at 9/8 H W runs.  The contract (csrc/mm_device.h, carve_workspace): a run beyond the list is dropped and reported like a
    record -- NaN in every texel of the image's texture gradient, never a short sum; nothing else changes.

    The mesh is the 20 480-face icosphere on its unperturbed template (smooth = 0.04), cameras at 1.9 and 3.4: the runs of an image are at most
    four per distinct visible face, and smpl_uv shows fewer than 1 100 faces at 64x64 from any distance (at most ~3 300 runs by the estimate
    against a list of 4 608: test_many_runs_within_the_list runs that batch), so the mesh the overflow needs is the finer one.  Host estimate:
    ~7 300 runs in the near image (over the list), ~2 400 in the far one (under it): the images that overflow, and only they, are loud."""
    case = _runs_case(pkg, gen_dir, "icosphere5", "spread", dist=[1.9, 3.4], smooth=0.04)
    new, old = case.pair()
    a, b = _arrays(new), _arrays(old)
    fidx_o, verdicts = _check_oracle(case, oracle, old, b, "run list overflow, two-pass step")
    assert all(v == "ok" for v in verdicts.values()), verdicts
    est, runcap, need, trcap = _run_numbers(case, new, fidx_o)
    print("estimated runs %s of %d, records needed %s of %d" % (est, runcap, need, trcap))
    assert max(need) <= trcap                                                # the record array holds every image's records
    over = [e >= 1.1 * runcap for e in est]
    assert over == [True, False] and est[1] * 1.1 <= runcap                   # each image clearly on one side of the list's capacity
    assert old.dropped_records() == [0, 0]
    dn = new.dropped_records()
    print("dropped records per image, step mode:", dn)
    assert [n > 0 for n in dn] == over
    gt_new, gt_old = a.pop("grad_textures"), b.pop("grad_textures")
    for i, o in enumerate(over):
        if o:
            assert bool(torch.isnan(gt_new[i]).all()), "image %d: %d texels of a poisoned gradient are not NaN" % (i, int((~torch.isnan(gt_new[i])).sum()))
        else:
            assert torch.equal(_bits(gt_new[i]), _bits(gt_old[i]))
    _same(a, b)


@pytest.mark.parametrize("name,uvs,kw", [("icosphere5", "one", dict(dist=[1.9, 3.4], smooth=0.04)), ("smpl_uv", "one", dict(dist=2.0)),
                                         ("smpl_uv", "spread", dict(dist=2.0))], ids=["control", "smpl_uv-control", "smpl_uv-spread"])
def test_many_runs_within_the_list(pkg, oracle, gen_dir, name, uvs, kw):
    """The controls of the overflow test.  Every face on ONE corner (the layout of the record-pool overflow tests): four runs per wave, the
    list far from full.  And smpl_uv at distance 2 with its faces spread over the 49 corners: dozens of runs per wave, about half the list.
    Step mode drops nothing, equals the two-pass step bit for bit, texture gradients included, and matches the oracle."""
    case = _runs_case(pkg, gen_dir, name, uvs, **kw)
    new, old = case.pair()
    a = _arrays(new)
    fidx_o, verdicts = _check_oracle(case, oracle, new, a, "%s, %s" % (name, uvs))
    est, runcap, need, trcap = _run_numbers(case, new, fidx_o)
    print("estimated runs %s of %d, records needed %s of %d" % (est, runcap, need, trcap))
    assert max(need) <= trcap and max(est) * 1.1 <= runcap                   # (hence max(est) < runcap: smpl_uv cannot fill the list at 64x64)
    if uvs == "one":
        assert max(est) <= 4 * 64
    else:
        assert min(est) >= 8 * 64                                            # more than the four runs per wave of the one-corner layout
    assert new.dropped_records() == [0, 0] and old.dropped_records() == [0, 0]
    assert bool(torch.isfinite(a["grad_textures"]).all())
    _same(a, _arrays(old))


# ---- 6. the soft mask away from its defaults ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("knum,boxlen,sigmainv", [(3, 0.02, 7000.0), (7, 0.08, 900.0)])
def test_non_default_soft_mask_in_step_mode(pkg, oracle, gen_dir, knum, boxlen, sigmainv):
    case = _Case(pkg, gen_dir, "sphere", 3, 32, seed=67, no_mask=False, soft_gt=True, soft=(knum, boxlen, sigmainv))
    new, old = case.pair()
    a = _arrays(new)
    _check_oracle(case, oracle, new, a, "sphere B=3 32x32 knum %d boxlen %.2f sigmainv %g" % (knum, boxlen, sigmainv))
    alpha = case.oracle_forward(oracle)[0][..., 3]
    assert ((alpha > 0.01) & (alpha < 0.99)).mean() > 0.005                  # there is a silhouette band to get wrong
    _same(a, _arrays(old))
