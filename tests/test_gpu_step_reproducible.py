"""The same step run again gives the same BITS: the render path holds no floating-point atomic, every sum is an integer sum or one taken in
a fixed order, and every hand-off between workgroups is a ticket (README).  tests/test_gpu_parity.py holds that at one shape,
smpl_uv_642 at 128x128; this file holds it at the smallest shapes that reach each distinct path of the step -- strips of a screen whose
bin lines are longer than a wave (the order workgroup's serial scans, csrc/mm_vertex.hip), the cooperative walk, a ragged screen with a
tail image, the largest mesh the vertex launch sorts, one shape on each side of that predicate -- and at the other entry points.

runs_equal builds n = 8 fresh steps on the same inputs, fills every step's workspace with a different byte (0x00, 0xAB, 0xFF, 0x5A in turn:
a result that depends on what the allocator left behind fails every time, not now and then), runs each once and requires every output, the
loss, all eight gradients and the `nheavy` pairs equal to run 0's bit for bit; then it runs step 1 a second time on its own workspace (the
tickets and cursors of its first run must have been reset).  Eight runs: with two equally likely outcomes, as the record of the 1024x64
strip shows (profiles/step_reproducibility.md), eight runs of a drifting step all agree once in 128.

Every case asserts the path it was built for (the bin grid, order_in_vertex, step_mode_taken, the `nheavy` pairs): it cannot pass on
another one."""
import importlib

import numpy as np
import pytest
import torch

from parity_bar import grad_close, rel_errors
from test_gpu_fused_step import LEAVES, _arrays, _same, _tile_counts
from test_gpu_order_in_vertex import HEAVY_CAND, _batch, _render
from test_step_plan_host import gen_dir  # noqa: F401  (the fixture the generated template is written under)

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xAB, 0xFF, 0x5A)
GRADS = tuple("grad_" + k for k in LEAVES)


# ---- the library's shape predicates, restated (csrc/mm_device.h) ---------------------------------------------------------------------------
def bin_shift_for(H, W, F):
    words, A = (F + 63) // 64, 140 * F + 128 * H * W
    for s in (3, 4):
        nb = ((W + (1 << s) - 1) >> s) * ((H + (1 << s) - 1) >> s)
        if nb * words * 8 * 16 <= A:
            return s
    return 5


def tile_slots(H, W):
    return 4 * ((W + 15) // 16) * ((H + 15) // 16)


def order_in_vertex(H, W, F):
    return tile_slots(H, W) <= 1024 and (F + 63) // 64 <= 64 and bin_shift_for(H, W, F) == 3


def bins(dr):
    s = bin_shift_for(dr.render_height, dr.image_size, dr.num_faces)
    return ((dr.image_size + (1 << s) - 1) >> s, (dr.render_height + (1 << s) - 1) >> s)


def _dev(att, gt):
    dev = torch.device("cuda:0")
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in att.items()}, gt.to(dev)


def _checked(a, grads=GRADS):
    """every compared gradient is there and is not all zero; face_idx holds covered and uncovered pixels"""
    for k in grads:
        assert k in a and float(a[k].abs().max()) > 0, k
    assert bool((a["face_idx"] >= 0).any()) and bool((a["face_idx"] < 0).any())


def runs_equal(make_step, n=8):
    """n fresh steps from make_step(), each on a workspace filled with another byte; every array and the nheavy pairs of every run equal to run 0's,
    and a second run of step 1 on its own workspace equal too.  Returns (run 0's arrays, its nheavy pairs (B,2), step 0)."""
    steps = [make_step() for _ in range(n)]
    got = []
    for i, st in enumerate(steps):
        st.ws.fill_(FILLS[i % len(FILLS)])
        st.run()
        got.append((_arrays(st), _tile_counts(st)[:, :2].copy()))
    a0, c0 = got[0]
    _checked(a0)
    for i, (a, c) in enumerate(got[1:], 1):
        try:
            _same(a0, a)
        except AssertionError as e:
            raise AssertionError("run %d (workspace filled with 0x%02X) against run 0: %s" % (i, FILLS[i % len(FILLS)], e))
        assert np.array_equal(c0, c), "nheavy pairs of run %d: %s, of run 0: %s" % (i, c.tolist(), c0.tolist())
    steps[1].run()                                                  # on its own workspace, as the first run left it
    try:
        _same(a0, _arrays(steps[1]))
    except AssertionError as e:
        raise AssertionError("the second run on the same workspace: %s" % e)
    assert np.array_equal(c0, _tile_counts(steps[1])[:, :2])
    return a0, c0, steps[0]


def _stepper(pkg, dr, att, gt, step_mode=True, options=0):
    stepmod = importlib.import_module("3d-magic-mirror_amd.step")
    att, gt = _dev(att, gt)

    def make():
        dr.options = options
        st = stepmod.RenderLossStep(dr, att, gt, no_mask=True, emit_imnormal=True, fused=True, step_mode=step_mode)
        dr.options = 0
        assert st.d.options == options
        return st
    return make


# ---- 1. strips: lines of bins longer than a wave, the sort in the vertex launch ------------------------------------------------------------------
STRIPS = [
    # name, B, S, ratio, (W, H), bins, camera distances (None: as drawn)
    ("smpl_uv_642", 1, 1024, 1.0 / 16, (1024, 64), (128, 8), [2.2]),        # the configuration on record (profiles/step_reproducibility.md)
    ("smpl_uv_642", 1, 64, 16, (64, 1024), (8, 128), [2.2]),                # a thread per column
    ("smpl_uv_642", 1, 520, 16.0 / 520, (520, 16), (65, 2), [2.2]),         # the smallest grid one bin past a wave
    ("sphere", 2, 520, 16.0 / 520, (520, 16), (65, 2), None),
    ("smpl_uv_642", 1, 16, 520.0 / 16, (16, 520), (2, 65), [2.2]),          # the same on the other axis
    ("sphere", 2, 16, 520.0 / 16, (16, 520), (2, 65), None),
    ("smpl_uv_642", 1, 512, 0.25, (512, 128), (64, 16), [2.2]),             # the control: a wave per line, clean on record
    ("smpl_uv_642", 1, 896, 64.0 / 896, (896, 64), (112, 8), [2.2]),        # drifted before the fix (one run of eight apart), as did ...
    ("smpl_uv_642", 1, 128, 1, (128, 128), (16, 16), [2.2]),                # ... two squares, no strips at all: four runs against four, and ...
    ("smpl_uv_642", 1, 96, 1, (96, 96), (12, 12), [2.2]),                   # ... the smallest screen found (one of eight; 64x64 and below held)
]


def _strip(pkg, name, B, S, ratio, screen, grid, dist, seed=61):
    dr = _render(pkg, name, S, ratio=ratio)
    assert (dr.image_size, dr.render_height) == screen
    assert bin_shift_for(screen[1], screen[0], dr.num_faces) == 3 and bins(dr) == grid      # 8-pixel bins (very thin screens get wider ones)
    assert tile_slots(screen[1], screen[0]) <= 1024 and (dr.num_faces + 63) // 64 <= 64
    assert order_in_vertex(screen[1], screen[0], dr.num_faces)
    att, gt = _batch(pkg, dr, B, seed=seed, **({"distances": dist} if dist is not None else {}))
    return dr, att, gt


@pytest.mark.parametrize("name,B,S,ratio,screen,grid,dist", STRIPS, ids=["%s-B%d-%dx%d" % (c[0], c[1], c[4][0], c[4][1]) for c in STRIPS])
def test_strips(pkg, name, B, S, ratio, screen, grid, dist):
    dr, att, gt = _strip(pkg, name, B, S, ratio, screen, grid, dist)
    a, cn, st = runs_equal(_stepper(pkg, dr, att, gt))
    assert st.step_mode_taken()
    assert (max(grid) > 64) == (screen not in ((512, 128), (128, 128), (96, 96)))   # the serial scans: every strip but the control and the squares
    assert (cn[:, 1] > 0).all()
    print("%s %dx%d nheavy pairs %s" % (name, screen[0], screen[1], cn.tolist()))


# ---- 2. the cooperative walk ------------------------------------------------------------------------------------------------------------
def test_cooperative_walk(pkg):
    """test_gpu_order_in_vertex.test_cooperative_walk_is_taken's input: smpl_uv_642 at 64x64 from distances 10 and 16"""
    dr = _render(pkg, "smpl_uv_642", 64)
    att, gt = _batch(pkg, dr, 2, seed=35, distances=[10.0, 16.0])
    a, cn, st = runs_equal(_stepper(pkg, dr, att, gt))
    assert st.step_mode_taken() and order_in_vertex(64, 64, dr.num_faces)
    assert (cn[:, 0] >= 1).all(), "no tile with %d candidates: the cooperative walk was not taken (%s)" % (HEAVY_CAND, cn.tolist())


# ---- 3. a ragged screen with a tail image ---------------------------------------------------------------------------------------------------
def test_ragged_screen_tail_image(pkg):
    dr = _render(pkg, "sphere", 40, ratio=0.6)
    assert (dr.render_height, dr.image_size) == (24, 40)
    att, gt = _batch(pkg, dr, 3, seed=21)
    a, cn, st = runs_equal(_stepper(pkg, dr, att, gt))
    assert st.step_mode_taken() and st.B == 3 and st.B % 8 != 0      # (map_block's tail branch; partial bins and a partial 16x16 block)
    assert (cn[:, 1] > 0).all()


# ---- 4. the largest mesh the predicate takes --------------------------------------------------------------------------------------------------
def test_largest_sorted_mesh(pkg, gen_dir):
    dr = _render(pkg, "latlong4096", 48, gen=gen_dir)
    assert dr.num_faces == 4096 and order_in_vertex(48, 48, 4096) and not order_in_vertex(48, 48, 4097)
    att, gt = _batch(pkg, dr, 2, seed=39)
    a, cn, st = runs_equal(_stepper(pkg, dr, att, gt))
    assert st.step_mode_taken() and (cn[:, 1] > 0).all()


# ---- 5. one shape on each side of the predicate -----------------------------------------------------------------------------------------------
def test_more_than_1024_tile_slots(pkg):
    """257x256: seventeen blocks across, 1 088 tile slots -- the smallest screen above 1 024 slots that is one block wider than a square of
    them; the sort runs in a launch of its own (bincount_kernel + order_kernel), the step stays in step mode."""
    dr = _render(pkg, "sphere", 257, ratio=256.0 / 257)
    H, W = dr.render_height, dr.image_size
    assert (W, H) == (257, 256) and tile_slots(H, W) == 1088 and tile_slots(256, 256) == 1024
    assert bin_shift_for(H, W, dr.num_faces) == 3 and not order_in_vertex(H, W, dr.num_faces)
    att, gt = _batch(pkg, dr, 1, seed=63)
    a, cn, st = runs_equal(_stepper(pkg, dr, att, gt))
    assert st.step_mode_taken() and cn[0, 1] > 16


def test_bins_wider_than_eight_pixels(pkg):
    """smpl_uv (13 776 faces, 216 mask words): the smallest square screen in steps of a bin that bin_shift_for gives 16-pixel bins is 80x80 (72x72
    still gets 8-pixel ones; meshes of at most 4 096 faces keep 8-pixel bins on every screen more than a few pixels high).  The compacting
    walk, face flags, the standalone pixel backward: not a step-mode shape."""
    F = 13776
    assert [s for s in range(8, 129, 8) if bin_shift_for(s, s, F) != 3][0] == 80
    dr = _render(pkg, "smpl_uv", 80)
    assert dr.num_faces == F and bin_shift_for(80, 80, F) == 4 and not order_in_vertex(80, 80, F)
    att, gt = _batch(pkg, dr, 1, seed=65)
    a, cn, st = runs_equal(_stepper(pkg, dr, att, gt))
    assert not st.step_mode_taken() and cn[0, 1] > 0


# ---- 6. the other entry points, at 1024x64 and at one ordinary shape -----------------------------------------------------------------------
ENTRY_SHAPES = [("smpl_uv_642", 1024, 1.0 / 16, (1024, 64), [2.2]), ("sphere", 48, 1, (48, 48), None)]
ENTRY_IDS = ["1024x64", "48x48"]


@pytest.mark.parametrize("name,S,ratio,screen,dist", ENTRY_SHAPES, ids=ENTRY_IDS)
def test_step_without_step_mode(pkg, name, S, ratio, screen, dist):
    dr = _render(pkg, name, S, ratio=ratio)
    assert (dr.image_size, dr.render_height) == screen
    att, gt = _batch(pkg, dr, 1 if dist else 2, seed=67, **({"distances": dist} if dist else {}))
    a, cn, st = runs_equal(_stepper(pkg, dr, att, gt, step_mode=False))
    assert not st.step_mode_taken() and (cn[:, 1] > 0).all()


def _api_runs_equal(run, n=8):
    """an entry point that does not expose its workspace: n runs on fresh tensors, everything equal to run 0 bit for bit"""
    got = [run() for _ in range(n)]
    _checked(got[0], grads=[k for k in got[0] if k.startswith("grad_")])
    assert sum(k.startswith("grad_") for k in got[0]) == 8
    for i, a in enumerate(got[1:], 1):
        try:
            _same(got[0], a)
        except AssertionError as e:
            raise AssertionError("run %d against run 0: %s" % (i, e))
    return got[0]


def _leaves(att, dev, keys=LEAVES):
    return {k: (v.to(dev).clone().requires_grad_(k in keys) if torch.is_tensor(v) else v) for k, v in att.items()}


def _collect(rgbs, face_idx, out, datt):
    torch.cuda.synchronize()
    a = {"rgba": rgbs.detach().clone(), "face_idx": face_idx.clone(), "face_normals": out["face_normals"].detach().clone()}
    a.update({"grad_" + k: datt[k].grad.detach().clone() for k in LEAVES})
    return a


@pytest.mark.parametrize("name,S,ratio,screen,dist", ENTRY_SHAPES, ids=ENTRY_IDS)
def test_autograd_route(pkg, name, S, ratio, screen, dist):
    """dr.render followed by recon_data(...).backward()"""
    dev = torch.device("cuda:0")
    dr = _render(pkg, name, S, ratio=ratio)
    att, gt = _batch(pkg, dr, 1 if dist else 2, seed=69, **({"distances": dist} if dist else {}))
    gtd = gt.to(dev)

    def run():
        datt = _leaves(att, dev)
        rgbs, out = dr.render(no_mask=True, **datt)
        loss = dr.recon_data(rgbs, gtd, no_mask=True)
        loss.backward()
        a = _collect(rgbs, dr.last_face_idx, out, datt)
        a["loss"] = loss.detach().clone()
        return a
    _api_runs_equal(run)


@pytest.mark.parametrize("name,S,ratio,screen,dist", ENTRY_SHAPES, ids=ENTRY_IDS)
def test_render_views_two_views(pkg, name, S, ratio, screen, dist):
    dev = torch.device("cuda:0")
    dr = _render(pkg, name, S, ratio=ratio)
    B = 1 if dist else 2
    att, gt = _batch(pkg, dr, B, seed=71, **({"distances": dist} if dist else {}))
    att = dict(att)
    for k in ("azimuths", "elevations", "distances", "biases"):
        att[k] = att[k][:, None].repeat(1, 2, *([1] * (att[k].dim() - 1))).contiguous()
    att["azimuths"] = att["azimuths"] + torch.tensor([0.0, 90.0])
    w = torch.from_numpy(np.random.default_rng(5).normal(size=(B, 2, 4, dr.render_height, dr.image_size)).astype(np.float32)).to(dev)

    def run():
        datt = _leaves(att, dev)
        rgbs, out = dr.render_views(no_mask=True, **datt)
        assert rgbs.shape[:2] == (B, 2)
        (rgbs * w).sum().backward()
        return _collect(rgbs, dr.last_face_idx, out, datt)
    _api_runs_equal(run)


@pytest.mark.parametrize("name,S,ratio,screen,dist", ENTRY_SHAPES, ids=ENTRY_IDS)
def test_render_indexed_repeated_row(pkg, name, S, ratio, screen, dist):
    """three images over two rows of every indexed tensor, row 0 read twice: its gradient is a sum of two images' in ascending order"""
    dev = torch.device("cuda:0")
    dr = _render(pkg, name, S, ratio=ratio)
    M, idx = 3, [0, 1, 0]
    att, gt = _batch(pkg, dr, M, seed=73, **({"distances": [2.2, 2.4, 2.0]} if dist else {}))
    att = dict(att)
    for k in ("vertices", "textures", "lights", "bg"):
        att[k] = att[k][:2].contiguous()
    index = {k: torch.tensor(idx, dtype=torch.int64, device=dev) for k in ("vertices", "textures", "lights", "bg")}
    w = torch.from_numpy(np.random.default_rng(7).normal(size=(M, 4, dr.render_height, dr.image_size)).astype(np.float32)).to(dev)

    def run():
        datt = _leaves(att, dev)
        rgbs, out = dr.render_indexed(no_mask=True, index=index, **datt)
        (rgbs * w).sum().backward()
        return _collect(rgbs, dr.last_face_idx, out, datt)
    _api_runs_equal(run)


# ---- which bits are right: the thin strips against the float64 oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("S,ratio,screen,dist", [(520, 16.0 / 520, (520, 16), [1.2, 1.3]), (16, 520.0 / 16, (16, 520), [1.9, 2.1])], ids=["520x16", "16x520"])
def test_thin_strips_match_the_oracle(pkg, oracle, S, ratio, screen, dist):
    """The step at 520x16 and 16x520 (sphere, B = 2, cameras close enough that faces span several pixels) against the CPU oracle: face_idx
    bit-exact, the image within 1e-4, the loss within 1e-5, every gradient within 1e-4 of its own maximum (parity_bar.grad_close; where the
    fp32 oracle is itself farther than that from its float64 form, parity_bar's conditioning rule decides, as in tests/test_gpu_parity.py).
    Distances: at 520x16 the sphere is as high as the screen from 1.2 and 1.3 (6 % of the pixels covered, four to six pixels a face; from 2
    it covers 2.5 %); at 16x520 the projection stretches x by 32.5, and from 1.9 and 2.1 the sphere fills 92 % of the screen, hundreds of
    pixels a face, with uncovered pixels left at the ends."""
    dr, att, gt = _strip(pkg, "sphere", 2, S, ratio, screen, bins(_render(pkg, "sphere", S, ratio=ratio)), dist, seed=75)
    W, H = screen
    st = _stepper(pkg, dr, att, gt)()
    st.ws.fill_(0xAB)
    st.run()
    a = _arrays(st)
    inp = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in att.items()}
    inp["faces"] = dr.faces.numpy().astype(np.int32)
    inp["face_uvs"] = dr.face_uvs.numpy()[0]
    proj = dr.cam_proj.numpy().reshape(3)
    rgba_o, fidx_o, fn_o, imn_o = oracle.render_forward(inp, H, W, True, proj)
    loss_o, dpred = oracle.recon_data(rgba_o.transpose(0, 3, 1, 2), gt.numpy(), image_weight=dr.image_weight, want_grad=True)
    dp = np.ascontiguousarray(dpred.transpose(0, 2, 3, 1))
    g_o = oracle.render_backward(inp, H, W, True, proj, dp)
    g64 = {}

    def ref64(k):
        if not g64:
            g64.update(oracle.render_backward(inp, H, W, True, proj, dp.astype(np.float64), dtype=np.float64))
        return g64[k]
    fidx = a["face_idx"].cpu().numpy()
    assert (fidx == fidx_o).all(), "face_idx mismatches: %d" % int((fidx != fidx_o).sum())
    cover = float((fidx >= 0).mean())
    print("%dx%d covered %.3f" % (W, H, cover))
    assert cover > 0.03
    err = float(np.abs(a["rgba"].cpu().numpy() - rgba_o).max())
    assert err <= 1e-4 * max(1.0, float(np.abs(rgba_o).max())), err
    assert abs(float(a["loss"]) - loss_o) < 1e-5
    verdicts = {k: grad_close(a["grad_" + k], g_o[k], rtol=1e-4, what="%dx%d, %s" % (W, H, k), ref64=lambda k=k: ref64(k)) for k in LEAVES}
    print("%dx%d verdicts %s" % (W, H, verdicts))
    for k, v in verdicts.items():                                   # (a conditioning case: the distances the rule weighed, for the record)
        if v == "cond":
            print("%dx%d %s: of the maximum, HIP - fp32 oracle %.3e, fp32 oracle - float64 %.3e, HIP - float64 %.3e" % (
                W, H, k, rel_errors(a["grad_" + k], g_o[k])[0], rel_errors(g_o[k], ref64(k))[0], rel_errors(a["grad_" + k], ref64(k))[0]))
    assert all(float(np.abs(g_o[k]).max()) > 0 for k in LEAVES)
