"""The row sum that ends the backward of DiffRender.render_views and DiffRender.render_indexed (csrc/mm_row_sum.h), at its edges, through the
class API only.

The yardstick is never the sum itself: ``DiffRender.render`` on leaves that were EXPLICITLY replicated or gathered (index_select) gives the
per-image gradients g, and the expected gradient of a shared row is the adds written out here, in fp32 on the device, in ascending image
order -- acc = g[list[0]], then acc = acc + g[m] -- and zeros for a row no image reads.  Every comparison is torch.equal.

What the cases walk through: sums of 1 (no launch), 2 (one trip, one row), 3 (one full trip), 4 and 5 rows (a full trip and a half / two) and
of none; lists that ascend without being consecutive; rows of 1152 sixteen-byte units (one workgroup's 1024 and 128 more), of exactly
3 x 1024 units, of 4107 floats (not a multiple of four: 4-byte units, five workgroups, the last with 11 units), of 1926 floats (4-byte units,
1024 + 902) and of 9.  An output or staging pointer that is not 16-byte aligned cannot be reached through the class API (the node
allocates the gradients, the staging areas are 256-byte aligned): that fallback rests on the one `vec` predicate of row_sum_pack."""
import os

import pytest
import torch

from conftest import TEMPLATES

pytestmark = pytest.mark.gpu
SHARED = ("vertices", "textures", "lights", "bg")
CAMERAS = ("azimuths", "elevations", "distances", "biases")
_RENDERERS = {}


def _renderer(pkg, S):
    if S not in _RENDERERS:
        _RENDERERS[S] = pkg.DiffRender(os.path.join(TEMPLATES, "smpl_uv_642.npz"), S, emit_imnormal=False)
    return _RENDERERS[S]


def _inputs(pkg, dr, M, rows, S, tex, seed):
    """CPU tensors: rows[k] rows of the shared tensor k (textures of size `tex`), cameras for M images, an upstream gradient of the image"""
    att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, max([M] + list(rows.values())), S, S, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    att["textures"] = torch.rand(att["textures"].shape[0], 3, tex[0], tex[1], generator=g)
    own = {k: att[k][:rows[k]].contiguous() for k in SHARED}
    own.update({c: att[c][:M].contiguous() for c in CAMERAS})
    return own, torch.randn(M, 4, S, S, generator=g)


def _written_out(g, lists):
    """the expected gradient of every row: the per-image gradients g (M, ...) added in the list's order, the first one starting the sum"""
    out = torch.zeros((len(lists),) + tuple(g.shape[1:]), device=g.device, dtype=g.dtype)
    for r, lst in enumerate(lists):
        if lst:
            acc = g[lst[0]].clone()
            for m in lst[1:]:
                acc = acc + g[m]
            out[r] = acc
    return out


def _per_image_grads(dr, own, lists, w, dev):
    """plain render on the gathered leaves: image i reads row index[k][i] of tensor k"""
    M = w.shape[0]
    gat = {}
    for k in SHARED:
        index = torch.empty(M, dtype=torch.long)
        for r, lst in enumerate(lists[k]):
            index[lst] = r
        gat[k] = own[k].to(dev).index_select(0, index.to(dev)).contiguous().requires_grad_(True)
    gat.update({c: own[c].to(dev).requires_grad_(True) for c in CAMERAS})
    rgbs, _ = dr.render(no_mask=True, **gat)
    (rgbs * w).sum().backward()
    return {k: gat[k].grad for k in SHARED}, rgbs.detach()


def _sentinel(leaves):
    """Best effort: two NaN-filled blocks of every leaf's size are freed just before the backward, so that the caching allocator hands them to the
    node's empty_like of the gradients and an empty row left unwritten would read NaN.  The class API gives no way to force or to verify that
    reuse; where the allocator hands out fresh blocks instead, the empty-row assertion of _check is zeros-only (it cannot tell written zeros
    from a fresh block's)."""
    junk = [torch.full_like(t, float("nan")) for t in leaves.values() for _ in range(2)]
    torch.cuda.synchronize()
    del junk


def _check(got, g, lists, what):
    for k in SHARED:
        want = _written_out(g[k], lists[k])
        assert float(want.abs().max()) > 0, (what, k)
        assert torch.equal(got[k], want), (what, k, float((got[k] - want).abs().max()))
        for r, lst in enumerate(lists[k]):
            if not lst:
                assert int(torch.count_nonzero(got[k][r])) == 0, (what, k, r)


def _views_case(pkg, S, B, N, tex, seed):
    dev = torch.device("cuda:0")
    dr = _renderer(pkg, S)
    rows = {k: B for k in SHARED}
    own, w = _inputs(pkg, dr, B * N, rows, S, tex, seed)
    lists = {k: [[b * N + v for v in range(N)] for b in range(B)] for k in SHARED}
    g, ref = _per_image_grads(dr, own, lists, w.to(dev), dev)
    leaves = {k: own[k].to(dev).requires_grad_(True) for k in SHARED}
    cams = {c: own[c].to(dev).reshape((B, N) + tuple(own[c].shape[1:])) for c in CAMERAS}
    rgbs, _ = dr.render_views(no_mask=True, **leaves, **cams)
    assert torch.equal(rgbs.reshape(ref.shape), ref)
    _sentinel(leaves)
    (rgbs * w.to(dev).reshape(rgbs.shape)).sum().backward()
    _check({k: leaves[k].grad for k in SHARED}, g, lists, "render_views N=%d" % N)


def _indexed_case(pkg, S, M, lists, tex, seed):
    dev = torch.device("cuda:0")
    dr = _renderer(pkg, S)
    rows = {k: len(lists[k]) for k in SHARED}
    own, w = _inputs(pkg, dr, M, rows, S, tex, seed)
    g, ref = _per_image_grads(dr, own, lists, w.to(dev), dev)
    leaves = {k: own[k].to(dev).requires_grad_(True) for k in SHARED}
    cams = {c: own[c].to(dev) for c in CAMERAS}
    index = {}
    for k in SHARED:
        index[k] = torch.empty(M, dtype=torch.int32)
        for r, lst in enumerate(lists[k]):
            index[k][lst] = r
    rgbs, _ = dr.render_indexed(no_mask=True, index={k: v.to(dev) for k, v in index.items()}, **leaves, **cams)
    assert torch.equal(rgbs, ref)
    _sentinel(leaves)
    (rgbs * w.to(dev)).sum().backward()
    _check({k: leaves[k].grad for k in SHARED}, g, lists, "render_indexed")
    assert dr.poll_dropped_records() == 0


def _interleaved(counts):
    """lists with the given lengths over sum(counts) images, dealt round-robin, the longest list first in every round: every list ascends and
    no two of its images are neighbours"""
    lists, left, i = [[] for _ in counts], list(counts), 0
    order = sorted(range(len(counts)), key=lambda r: -counts[r])
    while any(left):
        for r in order:
            if left[r]:
                lists[r].append(i)
                left[r] -= 1
                i += 1
    for lst in lists:
        assert all(b - a > 1 for a, b in zip(lst, lst[1:])), lists
    return lists


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_view_sums_of_one_to_four_rows(pkg, N):
    _views_case(pkg, 32, 2, N, (64, 32), seed=10 + N)


def test_index_sums_of_none_to_five_rows(pkg):
    """15 images over 6 rows of every tensor, read by 0, 1, 2, 3, 4 and 5 images; which row gets which length differs per tensor"""
    counts = {"vertices": [0, 1, 2, 3, 4, 5], "textures": [3, 5, 0, 4, 1, 2], "lights": [5, 2, 4, 0, 3, 1], "bg": [1, 4, 3, 5, 2, 0]}
    _indexed_case(pkg, 32, 15, {k: _interleaved(c) for k, c in counts.items()}, (64, 32), seed=20)


# (image size, texture size): what the rows' lengths are in 16-byte or 4-byte units
UNIT_EDGES = {"textures 1152 units: a chunk and 128": (32, (32, 48)), "textures 4107 floats: 4-byte units, the last chunk 11": (32, (37, 37)),
              "bg 3 x 1024 units exactly": (64, (32, 48))}


@pytest.mark.parametrize("S,tex", list(UNIT_EDGES.values()), ids=list(UNIT_EDGES))
def test_unit_and_chunk_edges(pkg, S, tex):
    """every case also has the vertices' 1926 floats (4-byte units, 1024 + 902) and the lights' 9"""
    dr = _renderer(pkg, S)
    assert dr.num_vertices * 3 == 1926 and dr.render_height == S
    _views_case(pkg, S, 2, 3, tex, seed=30)
    _indexed_case(pkg, S, 6, {k: _interleaved(c) for k, c in {"vertices": [3, 2, 1], "textures": [1, 3, 2], "lights": [2, 1, 3], "bg": [2, 3, 1]}.items()},
                  tex, seed=31)
