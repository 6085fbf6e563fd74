"""DiffRender.render_indexed on the GPU: M images in one pass, each reading the row of vertices, textures, lights and bg its index names.

The yardstick everywhere below is ``DiffRender.render`` on leaves that were EXPLICITLY GATHERED with index_select: the path the rest of the
suite holds to the oracle -- never render_indexed itself.  Forward outputs must be bit-identical (torch.equal); the per-image camera
gradients too; the gradient of an indexed tensor must equal, to the bit, a loop written out here and run in fp32 on the device over the
gathered path's per-image leaf gradients g:  acc = g[list[0]], then acc = acc + g[m] in ascending m, zeros for a row no image reads
(no index_add_, whose order is the atomics').  Every compared gradient has a non-zero maximum and at least 2 % of the pixels are covered.
One test anchors the whole against the CPU oracle at the suite's bars, so that the file does not only compare the project with itself."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import TEMPLATES
from parity_bar import grad_close

pytestmark = pytest.mark.gpu
SHARED = ("vertices", "textures", "lights", "bg")
CAMERAS = ("azimuths", "elevations", "distances", "biases")

# the mixed case: 11 images over 3 meshes, 5 textures, 1 light row, 2 backgrounds; non-monotone; texture rows read by 5, 1, 0, 3 and 2 images
# (the odd and the even tail of the sum's two-at-a-time loop, a single image, and the row of zeros)
MIXED_ROWS = {"vertices": 3, "textures": 5, "lights": 1, "bg": 2}
MIXED = {"vertices": [2, 0, 1, 1, 2, 0, 0, 2, 1, 0, 2], "textures": [3, 0, 4, 0, 1, 3, 0, 4, 0, 3, 0], "lights": [0] * 11,
         "bg": [1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1]}


class Case:
    """the two paths on the same numbers: `own` holds the (R,...) leaves render_indexed takes, `gat` the gathered (M,...) leaves of render"""

    def __init__(self, pkg, M, rows, index, S=64, ratio=1, no_mask=True, seed=0, name="sphere", imn=True, skip=()):
        self.dev = dev = torch.device("cuda:0")
        self.dr = dr = pkg.DiffRender(os.path.join(TEMPLATES, name + ".npz"), S, ratio=ratio, emit_imnormal=imn)
        self.M, self.rows, self.no_mask = M, dict(rows), no_mask
        self.H, self.W = dr.render_height, dr.image_size
        nb = max([M] + [rows[k] for k in SHARED if k != "lights"])
        att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, nb, self.H, self.W, seed=seed)
        if rows["lights"] > nb:                                   # (thousands of light rows: 9 floats each, the batch's own rows varied)
            R = rows["lights"]
            att["lights"] = att["lights"][torch.arange(R) % nb] + 0.02 * torch.randn(R, 9, generator=torch.Generator().manual_seed(seed))
        self.index = {k: (None if index.get(k) is None else [int(i) for i in index[k]]) for k in SHARED}      # None: the identity
        self.skip = set(skip)                                                                                 # bad images (left out of every sum)
        self.own = {k: att[k][:rows[k]].to(dev).contiguous().requires_grad_(True) for k in SHARED}
        self.own.update({c: att[c][:M].to(dev).contiguous().requires_grad_(True) for c in CAMERAS})
        self.gat = {}
        for k in SHARED:
            lst = self.lists(k)
            self.gat[k] = self.own[k].detach().index_select(0, torch.tensor(lst, device=dev)).contiguous().requires_grad_(True)
        self.gat.update({c: self.own[c].detach().clone().requires_grad_(True) for c in CAMERAS})
        if not no_mask:
            self.own["bg"] = self.gat["bg"] = None

    def lists(self, k):
        return list(range(self.M)) if self.index[k] is None else self.index[k]

    def index_arg(self, kind="device64"):
        out = {}
        for k in SHARED:
            if self.index[k] is None or (k == "bg" and not self.no_mask):
                continue
            if kind == "list":
                out[k] = list(self.index[k])
            elif kind == "cpu":
                out[k] = torch.tensor(self.index[k], dtype=torch.int64)
            else:
                out[k] = torch.tensor(self.index[k], dtype=torch.int32 if kind == "device32" else torch.int64, device=self.dev)
        return out

    def render_indexed(self, kind="device64", leaves=None):
        r, a = self.dr.render_indexed(no_mask=self.no_mask, index=self.index_arg(kind), **(leaves or self.own))
        return r, a, self.dr.last_face_idx

    def render_gathered(self):
        r, a = self.dr.render(no_mask=self.no_mask, **self.gat)
        return r, a, self.dr.last_face_idx

    def upstream(self, seed):
        g = torch.Generator().manual_seed(seed)
        w = torch.randn(self.M, 4, self.H, self.W, generator=g).to(self.dev)
        wfn = torch.randn(self.M, self.dr.num_faces, 3, generator=g).to(self.dev)
        return w, wfn

    def leaves(self):
        return [k for k in SHARED + CAMERAS if self.own[k] is not None]

    def zero_grads(self):
        for d in (self.own, self.gat):
            for t in d.values():
                if t is not None:
                    t.grad = None

    def check_forward(self, v, r):
        (rv, av, fv), (rr, ar, fr) = v, r
        M, H, W = self.M, self.H, self.W
        assert rv.shape == (M, 4, H, W) and rv.stride() == (H * W * 4, 1, W * 4, 4)              # the permuted view of NHWC memory
        assert fv.shape == (M, H, W) and av["face_normals"].shape == (M, self.dr.num_faces, 3)
        assert torch.equal(rv.detach(), rr.detach())
        assert torch.equal(fv, fr)
        assert float((fv >= 0).float().mean()) > 0.02
        assert torch.equal(av["face_normals"].detach(), ar["face_normals"].detach())
        if self.dr.emit_imnormal:
            assert av["imnormal"].shape == (M, H, W, 3) and torch.equal(av["imnormal"], ar["imnormal"])
        else:
            assert av["imnormal"] is None

    def loop_sum(self, k, g):
        """the written-out reference of the index sum: per row, the gathered path's per-image gradients added in ascending image order"""
        lst, R = self.lists(k), self.rows[k]
        out = torch.zeros((R,) + tuple(g.shape[1:]), device=g.device, dtype=torch.float32)
        readers = {}
        for m in range(self.M):                                                               # ascending m
            if m not in self.skip:
                readers.setdefault(lst[m], []).append(m)
        for r in range(R):
            ms = readers.get(r)
            if not ms:
                continue                                                                      # an unused row: zeros
            acc = g[ms[0]].clone()
            for m in ms[1:]:
                acc = acc + g[m]
            out[r] = acc
        return out

    def check_grads(self, what="", keys=None):
        for k in keys or self.leaves():
            got, ref = self.own[k].grad, self.gat[k].grad
            assert got is not None and ref is not None, (what, k)
            assert float(ref.abs().max()) > 0, (what, k)
            if k in CAMERAS:
                assert torch.equal(got, ref), (what, k)                                       # per image: the gathered path's bits
            else:
                want = self.loop_sum(k, ref)
                assert got.shape == self.own[k].shape and float(want.abs().max()) > 0, (what, k)
                assert torch.equal(got, want), (what, k, float((got - want).abs().max()), float(want.abs().max()))


def _backward_both(case, v, r, seed):
    w, wfn = case.upstream(seed)
    ((v[0] * w).sum() + (v[1]["face_normals"] * wfn).sum()).backward()
    ((r[0] * w).sum() + (r[1]["face_normals"] * wfn).sum()).backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("no_mask", [True, False])
def test_identity_equals_render(pkg, no_mask):
    """index=None with M = 4 at 64x64 (config 1's shape): render's bits, forward and every gradient"""
    case = Case(pkg, 4, dict.fromkeys(SHARED, 4), {}, no_mask=no_mask, seed=3)
    r, a = case.dr.render_indexed(no_mask=no_mask, index=None, **case.own)
    v = (r, a, case.dr.last_face_idx)
    g = case.render_gathered()
    case.check_forward(v, g)
    _backward_both(case, v, g, seed=17)
    case.check_grads("identity")
    for k in case.leaves():                                              # one image per row: the sum is the image's gradient itself
        assert torch.equal(case.own[k].grad, case.gat[k].grad), k
    assert len(case.leaves()) == (8 if no_mask else 7)


def test_the_views_pattern_equals_render_views(pkg):
    """index = arange(B).repeat_interleave(N), B = 3, N = 3: render_views' bits, its summed gradients included"""
    B, n = 3, 3
    idx = torch.arange(B).repeat_interleave(n).tolist()
    case = Case(pkg, B * n, dict.fromkeys(SHARED, B), dict.fromkeys(SHARED, idx), seed=5)
    v = case.render_indexed()
    views = {k: case.own[k].detach().clone().requires_grad_(True) for k in SHARED}
    views.update({c: case.own[c].detach().reshape((B, n) + tuple(case.own[c].shape[1:])).clone().requires_grad_(True) for c in CAMERAS})
    rv, av = case.dr.render_views(no_mask=True, **views)
    fv = case.dr.last_face_idx
    H, W = case.H, case.W
    assert torch.equal(v[0].detach(), rv.detach().reshape(B * n, 4, H, W)) and torch.equal(v[2], fv.reshape(B * n, H, W))
    assert torch.equal(v[1]["face_normals"].detach(), av["face_normals"].detach().reshape(B * n, -1, 3))
    assert float((fv >= 0).float().mean()) > 0.02
    w, wfn = case.upstream(9)
    ((v[0] * w).sum() + (v[1]["face_normals"] * wfn).sum()).backward()
    ((rv * w.reshape(B, n, 4, H, W)).sum() + (av["face_normals"] * wfn.reshape(B, n, -1, 3)).sum()).backward()
    torch.cuda.synchronize()
    for k in SHARED + CAMERAS:
        got, ref = case.own[k].grad, views[k].grad.reshape(case.own[k].shape)
        assert float(ref.abs().max()) > 0 and torch.equal(got, ref), k


@pytest.mark.parametrize("ratio", [1, 2], ids=["64x64", "Market 128x64"])
def test_mixed_indices(pkg, ratio):
    """M = 11 over 3 / 5 / 1 / 2 rows: the texture and bg rows are multiples of four floats (16-byte units), V*3 = 1926 and the 9 lights are not"""
    case = Case(pkg, 11, MIXED_ROWS, MIXED, ratio=ratio, seed=7, name="sphere" if ratio == 1 else "smpl_uv_642")
    assert case.own["textures"][0].numel() % 4 == 0 and case.own["vertices"][0].numel() == 1926
    v, g = case.render_indexed(), case.render_gathered()
    case.check_forward(v, g)
    _backward_both(case, v, g, seed=11)
    case.check_grads("mixed")
    assert int(torch.count_nonzero(case.own["textures"].grad[2])) == 0          # the row no image reads
    assert sorted(MIXED["textures"].count(r) for r in range(5)) == [0, 1, 2, 3, 5]


def test_the_plans_chunk_edge(pkg):
    """M = 260 images (one full chunk of 256 and four more) at 32x32 over 7 rows, indices (m * 5) % 7"""
    M, R = 260, 7
    idx = [(m * 5) % R for m in range(M)]
    case = Case(pkg, M, dict.fromkeys(SHARED, R), dict.fromkeys(SHARED, idx), S=32, seed=13, imn=False)
    v, g = case.render_indexed(), case.render_gathered()
    case.check_forward(v, g)
    _backward_both(case, v, g, seed=2)
    case.check_grads("chunk edge", keys=("textures", "vertices"))


@pytest.mark.parametrize("R", [8192, 8193], ids=["8192 rows: counters in LDS", "8193 rows: counters in the workspace"])
def test_the_plans_row_count_threshold(pkg, R):
    """the plan keeps the counters of up to 8192 rows in LDS and of more in the workspace: 20 images at 32x32 over R light rows on either side of
    the threshold -- the last row, the first, rows read twice and three times, thousands read by none"""
    M = 20
    idx = [R - 1, 0, 4097, R - 1, 17, 0, 4097, 8000, 1, 0, 255, 256, 17, 8191, 2, 3, R - 1, 5000, 6, 4097]
    rows = dict.fromkeys(SHARED, M)
    rows["lights"] = R
    case = Case(pkg, M, rows, {"lights": idx}, S=32, seed=29, imn=False)
    v, g = case.render_indexed(), case.render_gathered()
    case.check_forward(v, g)
    _backward_both(case, v, g, seed=6)
    case.check_grads("row threshold")
    used = sorted(set(idx))
    unused = torch.ones(R, dtype=torch.bool)
    unused[used] = False
    assert int(torch.count_nonzero(case.own["lights"].grad[unused.to(case.dev)])) == 0
    assert all(float(case.own["lights"].grad[r].abs().max()) > 0 for r in used)


def test_grid_helper_renders_the_rainbow_loop(pkg):
    """grid_index(3, 4): 3 textures x 4 shapes against the reference's nested loop (show_rainbow2.py:376-399), restated with repeat"""
    nt, ns = 3, 4
    row, col = pkg.grid_index(nt, ns)
    dev = torch.device("cuda:0")
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), 64)
    att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, ns, 64, 64, seed=19)
    Ae = {k: att[k].to(dev) for k in SHARED[:3] + CAMERAS}
    Ae["bg"] = None
    sheet = dict(Ae)
    sheet["textures"] = Ae["textures"][:nt]
    for c in CAMERAS:
        sheet[c] = Ae[c][col.to(dev)]
    rgbs, out = dr.render_indexed(index={"vertices": col, "lights": col, "textures": row}, **sheet)
    fidx = dr.last_face_idx
    assert rgbs.shape == (nt * ns, 4, 64, 64) and float((fidx >= 0).float().mean()) > 0.02
    for i in range(nt):
        A_tmp = dict(Ae)
        A_tmp["textures"] = Ae["textures"][i].unsqueeze(0).repeat(ns, 1, 1, 1)
        ref, _ = dr.render(**A_tmp)
        assert torch.equal(rgbs[i * ns:(i + 1) * ns], ref), i
        assert torch.equal(fidx[i * ns:(i + 1) * ns], dr.last_face_idx), i


def test_index_types_give_the_same_bits(pkg):
    case = Case(pkg, 11, MIXED_ROWS, MIXED, seed=7)
    w, wfn = case.upstream(3)
    runs = []
    for kind in ("device64", "device32", "cpu", "list"):
        case.zero_grads()
        r, a, f = case.render_indexed(kind)
        ((r * w).sum() + (a["face_normals"] * wfn).sum()).backward()
        torch.cuda.synchronize()
        runs.append((r.detach().clone(), f.clone(), {k: case.own[k].grad.clone() for k in case.leaves()}))
    assert float((runs[0][1] >= 0).float().mean()) > 0.02
    for kind, (r, f, gr) in zip(("device32", "cpu", "list"), runs[1:]):
        assert torch.equal(r, runs[0][0]) and torch.equal(f, runs[0][1]), kind
        for k in gr:
            assert float(gr[k].abs().max()) > 0 and torch.equal(gr[k], runs[0][2][k]), (kind, k)


def test_out_of_range_device_index(pkg):
    """one bad entry among 6 images: that image is NaN with face_idx -1, the other five are the gathered render's, no row's gradient contains the
    bad image, the status poll reports 1 and the next render_indexed raises"""
    M, bad = 6, 3
    rows = {"vertices": 3, "textures": 4, "lights": 2, "bg": 2}
    index = {"vertices": [0, 2, 1, 1, 0, 2], "textures": [3, 0, 1, 1, 0, 3], "lights": [0, 1, 1, 0, 0, 1], "bg": [1, 0, 0, 1, 1, 0]}
    case = Case(pkg, M, rows, index, seed=23, skip=(bad,))                 # (the gathered path reads valid rows everywhere)
    arg = case.index_arg("device64")
    arg["textures"] = arg["textures"].clone()
    arg["textures"][bad] = rows["textures"]                                # == the row count: out of range
    g = case.render_gathered()                                            # (first: every call of the object polls the status word)
    r, a = case.dr.render_indexed(no_mask=True, index=arg, **case.own)
    f = case.dr.last_face_idx
    good = [m for m in range(M) if m != bad]
    assert torch.isnan(r.detach()[bad]).all() and bool((f[bad] == -1).all())
    assert torch.equal(r.detach()[good], g[0].detach()[good]) and torch.equal(f[good], g[2][good])
    assert float((f[good] >= 0).float().mean()) > 0.02
    w, wfn = case.upstream(5)
    ((r * w).sum() + (a["face_normals"] * wfn).sum()).backward()
    ((g[0] * w).sum() + (g[1]["face_normals"] * wfn).sum()).backward()
    torch.cuda.synchronize()
    for k in SHARED:                                                      # the loop leaves the bad image out (Case.skip)
        want = case.loop_sum(k, case.gat[k].grad)
        assert float(want.abs().max()) > 0 and torch.equal(case.own[k].grad, want), k
        assert torch.isfinite(case.own[k].grad).all(), k
    for c in CAMERAS:
        assert torch.isnan(case.own[c].grad[bad]).all(), c
        assert torch.equal(case.own[c].grad[good], case.gat[c].grad[good]) and float(case.gat[c].grad[good].abs().max()) > 0, c
    assert case.dr.poll_dropped_records(reset=False) == 1
    with pytest.raises(RuntimeError, match="outside their tensor's rows"):
        case.dr.render_indexed(no_mask=True, index=case.index_arg(), **case.own)
    case.dr.render_indexed(no_mask=True, index=case.index_arg(), **case.own)   # (reported once)
    torch.cuda.synchronize()
    assert case.dr.poll_dropped_records() == 0


def test_two_backward_runs_of_one_graph_are_bit_identical(pkg):
    case = Case(pkg, 11, MIXED_ROWS, MIXED, ratio=2, seed=9, name="smpl_uv_642")
    r, a, _ = case.render_indexed()
    w, wfn = case.upstream(4)
    loss = (r * w).sum() + (a["face_normals"] * wfn).sum()
    runs = []
    for _ in range(2):
        case.zero_grads()
        loss.backward(retain_graph=True)
        torch.cuda.synchronize()
        runs.append({k: case.own[k].grad.clone() for k in case.leaves()})
    for k in runs[0]:
        assert float(runs[0][k].abs().max()) > 0 and torch.equal(runs[0][k], runs[1][k]), k


def test_no_host_synchronisation(pkg):
    case = Case(pkg, 11, MIXED_ROWS, MIXED, seed=2)
    w, wfn = case.upstream(1)
    arg = case.index_arg("device64")
    r, a = case.dr.render_indexed(no_mask=True, index=arg, **case.own)   # (the shape's first call: library, extension and descriptor caches are warm after it)
    ((r * w).sum() + (a["face_normals"] * wfn).sum()).backward()
    case.zero_grads()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            torch.ones(1, device=case.dev).item()
            raised = False
        except RuntimeError:
            raised = True
        if not raised:
            pytest.skip("this torch build does not raise on a synchronising call under set_sync_debug_mode('error')")
        r, a = case.dr.render_indexed(no_mask=True, index=arg, **case.own)
        ((r * w).sum() + (a["face_normals"] * wfn).sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert all(torch.isfinite(case.own[k].grad).all() for k in case.leaves())


def test_forward_only_call_keeps_no_staging(pkg):
    """no input requires grad: the node's workspace is the backward = 0 query, and the outputs are the mixed case's"""
    case = Case(pkg, 11, MIXED_ROWS, MIXED, seed=7)
    N = pkg._native
    plain = {k: v.detach() for k, v in case.own.items()}
    r, a, f = case.render_indexed(leaves=plain)
    asked = case.dr.last_indexed_workspace_bytes
    assert not r.requires_grad
    g = case.render_gathered()
    case.check_forward((r, a, f), g)
    Ht, Wt = case.own["textures"].shape[2:]
    vd = N.MMRenderIndexedDesc()
    proto = case.dr._proto(case.dr._static(case.dev), 11, True, Ht, Wt)[0]
    ctypes.memmove(ctypes.byref(vd), proto, len(proto))
    for t, k in enumerate(SHARED):
        vd.rows[t] = MIXED_ROWS[k]
    vd.backward = 0
    q0 = int(N.lib().mm_render_indexed_query_workspace(ctypes.byref(vd)))
    vd.backward = 1
    q1 = int(N.lib().mm_render_indexed_query_workspace(ctypes.byref(vd)))
    assert asked == q0 and q1 >= q0 + 4 * 11 * (1926 + 3 * Ht * Wt + 9 + 3 * 64 * 64)
    case.render_indexed()                                                # with leaves that require grad: the staging is there
    assert case.dr.last_indexed_workspace_bytes == q1
    with torch.no_grad():
        case.render_indexed()
    assert case.dr.last_indexed_workspace_bytes == q0


def test_anchor_against_the_oracle(pkg, oracle):
    """the mixed case against the CPU oracle on the inputs gathered on the host, at the suite's bars: face_idx exact, RGBA 1e-4, gradients within
    1e-4 of their own maximum -- per image for the cameras, the oracle's per-image gradients summed per row in float64 for the indexed inputs"""
    M, S = 11, 64
    case = Case(pkg, M, MIXED_ROWS, MIXED, seed=7)
    r, a, fidx = case.render_indexed()
    rng = np.random.default_rng(77)
    w = rng.normal(size=(M, S, S, 4)).astype(np.float32)
    wfn = rng.normal(size=(M, case.dr.num_faces, 3)).astype(np.float32)
    dev = case.dev
    ((r.permute(0, 2, 3, 1) * torch.from_numpy(w).to(dev)).sum() + (a["face_normals"] * torch.from_numpy(wfn).to(dev)).sum()).backward()
    torch.cuda.synchronize()
    inp = {k: case.own[k].detach().cpu().numpy()[np.asarray(MIXED[k])] for k in SHARED}
    inp.update({c: case.own[c].detach().cpu().numpy() for c in CAMERAS})
    inp["faces"] = case.dr.faces.numpy().astype(np.int32)
    inp["face_uvs"] = case.dr.face_uvs.numpy()[0]
    proj = case.dr.cam_proj.numpy().reshape(3)
    rgba_o, fidx_o, fn_o, _ = oracle.render_forward(inp, S, S, True, proj)
    assert (fidx.cpu().numpy() == fidx_o).all()
    assert (fidx_o >= 0).mean() > 0.03
    assert np.abs(r.detach().permute(0, 2, 3, 1).cpu().numpy() - rgba_o).max() <= 1e-4
    assert np.abs(a["face_normals"].detach().cpu().numpy() - fn_o).max() <= 1e-6
    g_o = oracle.render_backward(inp, S, S, True, proj, w, wfn)
    g64 = {}

    def ref64(k):
        if not g64:
            g64.update(oracle.render_backward(inp, S, S, True, proj, w.astype(np.float64), wfn.astype(np.float64), dtype=np.float64))
        return g64[k]

    def fold(k, g):                                                     # the oracle's per-image gradient, as render_indexed returns it
        g = np.asarray(g)
        if k not in SHARED:
            return g
        out = np.zeros((MIXED_ROWS[k],) + g.shape[1:], dtype=np.float64)
        np.add.at(out, np.asarray(MIXED[k]), g.astype(np.float64))
        return out
    for k in SHARED + CAMERAS:
        ref = fold(k, g_o[k])
        assert float(np.abs(ref).max()) > 0, k
        verdict = grad_close(case.own[k].grad, ref, rtol=1e-4, what="anchor, " + k, ref64=lambda k=k: fold(k, ref64(k)))
        assert verdict == "ok", (k, verdict)
