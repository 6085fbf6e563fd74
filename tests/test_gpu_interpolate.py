"""Attribute interpolation on the MI355X (csrc/mm_interp.hip) against torch's eager fp32 composition of the reference's block
(trainer.py:279-342, restated here), the numpy restatement of the resampling rule (tests/test_interpolate_host.py: resample_np) and,
where torch's own sums are not in fp32, float64."""
import importlib
import os
import random
import types

import numpy as np
import pytest
import torch

from conftest import TEMPLATES
from parity_bar import grad_close, rel_errors
from test_interpolate_host import resample_np

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
IP = importlib.import_module("3d-magic-mirror_amd.interpolate")
KEYS = IP.MIX_KEYS
# (V, Ht, Wt, H, W): BASELINE configs 2 and 3
CONFIG2, CONFIG3 = (642, 256, 128, 128, 128), (642, 512, 256, 256, 256)


def attrs(B, shape, seed=0, bg=True, dtypes=None):
    V, Ht, Wt, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)  # noqa: E731
    A = {"vertices": r(B, V, 3), "delta_vertices": 0.05 * r(B, V, 3), "textures": r(B, 3, Ht, Wt), "bg": r(B, 3, H, W) if bg else None,
         "lights": r(B, 9)}
    for k, dt in (dtypes or {}).items():
        A[k] = A[k].to(dt)
    return A


def alphas(B, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return tuple(torch.rand(s, generator=g, device=DEV) for s in ((B, 1, 1), (B, 1, 1, 1), (B, 1)))


def eager(A, ia, ib, a_s, a_t, a_l):
    """trainer.py:307-340: deep_copy by ia / ib (gather + clone), then the lerps, as torch evaluates them"""
    Aa = {k: (None if A[k] is None else A[k][ia].clone()) for k in KEYS}
    Ab = {k: (None if A[k] is None else A[k][ib].clone()) for k in KEYS}
    return {"vertices": a_s * Aa["vertices"] + (1 - a_s) * Ab["vertices"],
            "delta_vertices": a_s * Aa["delta_vertices"] + (1 - a_s) * Ab["delta_vertices"],
            "textures": a_t * Aa["textures"] + (1.0 - a_t) * Ab["textures"],
            "bg": None if A["bg"] is None else a_t * Aa["bg"] + (1.0 - a_t) * Ab["bg"],
            "lights": a_l * Aa["lights"] + (1.0 - a_l) * Ab["lights"]}


def weighted_sum(out, ws):
    return sum((out[k] * ws[k]).sum() for k in KEYS if out[k] is not None and k in ws)


def weights(out, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return {k: torch.randn(out[k].shape, generator=g, device=DEV) for k in KEYS if out[k] is not None}


# ---- 1 / 2: forward and backward against torch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,shape,bg", [(48, CONFIG2, True), (48, CONFIG2, False), (48, CONFIG3, True), (1, CONFIG2, True),
                                        (384, CONFIG2, True), (5, (7, 5, 3, 3, 2), True)])
def test_forward_and_backward_equal_torch_for_permutations(B, shape, bg):
    A = attrs(B, shape, seed=B, bg=bg)
    a = alphas(B)
    rng = np.random.default_rng(B)
    ia, ib = rng.permutation(B), rng.permutation(B)
    src = {k: (None if v is None else v.clone().requires_grad_()) for k, v in A.items()}
    ref_src = {k: (None if v is None else v.clone().requires_grad_()) for k, v in A.items()}
    out = IP.mix_attributes(src, ia, ib, *a)
    ref = eager(ref_src, torch.from_numpy(ia).to(DEV), torch.from_numpy(ib).to(DEV), *a)
    for k in KEYS:
        assert (out[k] is None) == (ref[k] is None) and (out[k] is None or torch.equal(out[k], ref[k])), k
    ws = weights(ref)
    weighted_sum(out, ws).backward()
    weighted_sum(ref, ws).backward()
    for k in KEYS:
        if src[k] is not None:
            assert torch.equal(src[k].grad, ref_src[k].grad), k


def test_half_and_strided_inputs():
    B = 48
    A = attrs(B, CONFIG2, seed=3, dtypes={"bg": torch.float16, "lights": torch.float16})
    A["textures"] = A["textures"].transpose(2, 3).contiguous().transpose(2, 3)          # same values, other strides
    assert not A["textures"].is_contiguous()
    a = alphas(B)
    rng = np.random.default_rng(0)
    ia, ib = rng.permutation(B), rng.permutation(B)
    src = {k: v.clone().requires_grad_() for k, v in A.items()}
    out = IP.mix_attributes(src, torch.from_numpy(ia).to(DEV), torch.from_numpy(ib).to(DEV), *a)
    ref = eager(A, torch.from_numpy(ia).to(DEV), torch.from_numpy(ib).to(DEV), *a)
    for k in KEYS:
        assert out[k].dtype == torch.float32 and torch.equal(out[k], ref[k]), k
    ws = weights(ref)
    weighted_sum(out, ws).backward()
    # torch would sum the fp16 sources' two branches in fp16: compare every gradient with float64 instead
    A64 = {k: v.detach().double().requires_grad_() for k, v in A.items()}
    weighted_sum(eager(A64, torch.from_numpy(ia).to(DEV), torch.from_numpy(ib).to(DEV), *(x.double() for x in a)),
                 {k: w.double() for k, w in ws.items()}).backward()
    for k in KEYS:
        assert src[k].grad.dtype == A[k].dtype
        e, _ = rel_errors(src[k].grad.double(), A64[k].grad)
        assert e <= (1e-3 if A[k].dtype == torch.float16 else 1e-6), (k, e)


# ---- 3: duplicated indices -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["half_collapsed", "all_one_source"])
def test_backward_with_duplicated_indices(case):
    B = 48
    A = attrs(B, CONFIG2, seed=9)
    a = alphas(B, seed=4)
    rng = np.random.default_rng(1)
    if case == "half_collapsed":
        good = np.arange(0, B, 2)
        ia, ib = rng.choice(good, B), rng.choice(good, B)
    else:
        ia = ib = np.full(B, 7)
    runs = []
    for _ in range(2):
        src = {k: v.clone().requires_grad_() for k, v in A.items()}
        out = IP.mix_attributes(src, ia, ib, *a)
        ws = weights(out)
        weighted_sum(out, ws).backward()
        runs.append({k: src[k].grad.clone() for k in KEYS})
    A64 = {k: v.double().requires_grad_() for k, v in A.items()}
    ref = eager(A64, torch.from_numpy(ia).to(DEV), torch.from_numpy(ib).to(DEV), *(x.double() for x in a))
    weighted_sum(ref, {k: w.double() for k, w in ws.items()}).backward()
    unused = np.setdiff1d(np.arange(B), np.union1d(ia, ib))
    for k in KEYS:
        assert torch.equal(runs[0][k], runs[1][k]), k                        # bitwise reproducible
        e, _ = rel_errors(runs[0][k], A64[k].grad)
        assert e <= 1e-6, (k, e)
        assert (runs[0][k][torch.from_numpy(unused).to(DEV)] == 0).all(), k  # rows nobody selected: exactly 0
    # only some outputs used: the other sources get no gradient
    src = {k: v.clone().requires_grad_() for k, v in A.items()}
    out = IP.mix_attributes(src, ia, ib, *a)
    (out["textures"].sum() + out["lights"].sum()).backward()
    assert src["textures"].grad is not None and src["lights"].grad is not None
    assert src["vertices"].grad is None and src["delta_vertices"].grad is None and src["bg"].grad is None


# ---- 4: resampling against the numpy restatement ---------------------------------------------------------------------------------
def _resample_case(dv, ia, ib, u):
    got = IP.resample_collapsed(torch.from_numpy(dv).to(DEV), torch.from_numpy(ia).to(DEV), torch.from_numpy(ib).to(DEV),
                                torch.from_numpy(u).to(DEV))
    exp = resample_np(dv, ia, ib, u)
    assert got[0].cpu().numpy().tolist() == exp[0].tolist()
    assert got[1].cpu().numpy().tolist() == exp[1].tolist()
    assert int(got[2]) == exp[2]
    return exp


def test_resampling_matches_the_numpy_rule():
    rng = np.random.default_rng(7)
    for B, V in ((48, 642), (384, 642), (1, 1), (1, 5), (3000, 2)):
        dv = (0.05 * rng.standard_normal((B, V, 3))).astype(np.float32)
        ia, ib = rng.permutation(B), rng.permutation(B)
        u = rng.random((2, B), dtype=np.float32)
        assert _resample_case(dv, ia, ib, u)[2] == 0                         # none bad: unchanged
        exp = _resample_case(dv, ia, ib, u)
        assert exp[0].tolist() == ia.tolist()
        bad = rng.random(B) < 0.4
        dv[bad, -1, :] = 1.0
        if 0 < bad.sum() < B:
            assert _resample_case(dv, ia, ib, u)[2] == bad.sum()             # some bad
        for uu in (np.zeros((2, B), np.float32), np.full((2, B), np.nextafter(np.float32(1), np.float32(0)), np.float32)):
            _resample_case(dv, ia, ib, uu)                                   # uniforms of 0 and of just below 1
        dv[:, -1, :] = 2.0
        exp = _resample_case(dv, ia, ib, u)                                  # every sample bad: unchanged, n_bad == B
        assert exp[2] == B and exp[0].tolist() == ia.tolist()


def test_resampling_threshold_edges():
    B = 6
    dv = np.zeros((B, 4, 3), np.float32)
    x = np.float32(1.2)                                                      # ((x + 0) + 0) / 3 == 0.4f exactly: not bad
    assert (x + np.float32(0)) / np.float32(3) == np.float32(0.4)
    dv[0, -1, 0] = x
    dv[1, -1, :] = np.nan                                                    # NaN: not bad
    dv[2, -1, 1] = np.nextafter(x, np.float32(2))                            # just above: bad
    ia, ib = np.arange(B), np.arange(B)[::-1].copy()
    exp = _resample_case(dv, ia, ib, np.random.default_rng(0).random((2, B), dtype=np.float32))
    assert exp[2] == 1


# ---- 5: out-of-range device indices ----------------------------------------------------------------------------------------------
def test_out_of_range_device_indices_give_nan_rows():
    B = 8
    big = attrs(B + 2, (10, 8, 8, 4, 4), seed=2)
    A = {k: v[1:B + 1] for k, v in big.items()}                             # rows -1 and B lie inside the allocation
    a = alphas(B)
    ia = torch.arange(B, device=DEV, dtype=torch.int32)                      # int32: passed to the kernel as they are
    ib = torch.arange(B, device=DEV, dtype=torch.int32).flip(0)
    ia[2], ib[5] = -1, B
    out = IP.mix_attributes(A, ia, ib, *a)
    ok = torch.ones(B, dtype=torch.bool)
    ok[[2, 5]] = False
    ref = eager(A, ia.long().clamp(0, B - 1), ib.long().clamp(0, B - 1), *a)
    for k in KEYS:
        assert torch.isnan(out[k][~ok.to(DEV)]).all(), k
        assert torch.equal(out[k][ok.to(DEV)], ref[k][ok.to(DEV)]), k


# ---- 6 / 7 / 8: the whole block ---------------------------------------------------------------------------------------------------
def opt(**kw):
    o = dict(hard=True, hard_range=20, inv=0, lambda_ic=0.1, azi_scope=360, bias_range=0.5, beta=0.0, bg=True)
    o.update(kw)
    return types.SimpleNamespace(**o)


ELEV, DIST = (0.0, 30.0), (2.0, 7.0)


def block(Ae, o, B):
    """trainer.py:279-342 as the reference runs it (the sync, numpy's resampling, deep_copy, the lerps)"""
    if o.hard:
        Ae90 = {k: (None if v is None else v.clone()) for k, v in Ae.items() if k in IP.COPY_KEYS}
        if random.random() > 0.5:
            Ae90["azimuths"] = -torch.empty(B, dtype=torch.float32, device=DEV).uniform_(o.hard_range, 180 - o.hard_range)
        else:
            Ae90["azimuths"] = -torch.empty(B, dtype=torch.float32, device=DEV).uniform_(0, 180)
        rand = torch.empty(B, dtype=torch.float32, device=DEV).uniform_(-1.0, 1.0)
        rand[rand < 0] = -1.0
        rand[rand >= 0] = 1.0
        Ae90["azimuths"] *= rand
    else:
        Ae90 = None
    mean_delta = torch.mean(torch.abs(Ae["delta_vertices"])[:, -1], dim=1)
    bad_index = np.argwhere(mean_delta.data.cpu().numpy() > 0.4)
    rand_a, rand_b = np.random.permutation(B), np.random.permutation(B)
    if o.inv == 0:
        good_index = np.setdiff1d(np.arange(B), bad_index)
        for i in bad_index:
            rand_a[np.argwhere(rand_a == i)] = np.random.choice(good_index, 1)
            rand_b[np.argwhere(rand_b == i)] = np.random.choice(good_index, 1)
    if o.lambda_ic <= 0:
        return Ae, Ae90, None
    Ai = {}
    torch.empty(B, dtype=torch.float32, device=DEV).uniform_(0.0, 1.0)
    Ai["azimuths"] = -torch.empty(B, dtype=torch.float32, device=DEV).uniform_(-o.azi_scope / 2, o.azi_scope / 2)
    Ai["elevations"] = torch.empty(B, dtype=torch.float32, device=DEV).uniform_(*ELEV)
    Ai["distances"] = torch.empty(B, dtype=torch.float32, device=DEV).uniform_(*DIST)
    Ai["biases"] = torch.empty((B, 2), dtype=torch.float32, device=DEV).uniform_(-o.bias_range, o.bias_range)
    a_t = torch.empty((B, 1, 1, 1), dtype=torch.float32, device=DEV).uniform_(0.0, 1.0)
    a_s = torch.empty((B, 1, 1), dtype=torch.float32, device=DEV).uniform_(0.0, 1.0)
    a_l = torch.empty((B, 1), dtype=torch.float32, device=DEV).uniform_(0.0, 1.0)
    A = dict(Ae)
    if not o.bg:
        A["bg"] = None
    Ai.update(eager(A, torch.LongTensor(rand_a).to(DEV), torch.LongTensor(rand_b).to(DEV), a_s, a_t, a_l))
    return Ai, Ae90, (rand_a, rand_b, a_s, a_t, a_l)


def seeded(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def full_attrs(B, seed, collapsed=()):
    A = attrs(B, CONFIG2, seed=seed)
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    A.update(azimuths=torch.rand(B, generator=g, device=DEV), elevations=torch.rand(B, generator=g, device=DEV),
             distances=torch.rand(B, generator=g, device=DEV), biases=torch.rand(B, 2, generator=g, device=DEV))
    for b in collapsed:
        A["delta_vertices"][b, -1, :] = 1.0
    return A


@pytest.mark.parametrize("kw", [{}, {"hard": False}, {"bg": False}, {"inv": 1}, {"lambda_ic": 0.0}, {"hard": False, "inv": 1, "bg": False}])
def test_interpolate_attributes_equals_the_block_without_collapse(kw):
    B, o = 48, opt(**kw)
    Ae = full_attrs(B, seed=11)
    seeded(3)
    Ai, Ae90 = IP.interpolate_attributes(Ae, o, ELEV, DIST)
    seeded(3)
    Ri, R90, _ = block(Ae, o, B)
    if o.lambda_ic <= 0:
        assert Ai is Ae
    else:
        assert set(Ai) == set(Ri)
        for k, v in Ri.items():
            assert (v is None and Ai[k] is None) or torch.equal(Ai[k], v), k
    if not o.hard:
        assert Ae90 is None
    else:
        assert set(Ae90) == set(R90) and torch.equal(Ae90["azimuths"], R90["azimuths"])
        for k in IP.COPY_KEYS:
            if k != "azimuths" and k in Ae:
                assert Ae90[k] is Ae[k]                                          # the same tensors: render only reads them


def test_interpolate_attributes_resamples_collapsed_samples_by_the_rule():
    B, o = 48, opt()
    collapsed = (0, 5, 17, 40)
    Ae = full_attrs(B, seed=12, collapsed=collapsed)
    gen = torch.Generator(device=DEV).manual_seed(99)
    seeded(4)
    Ai, _ = IP.interpolate_attributes(Ae, o, ELEV, DIST, generator=gen)
    # the reference's draws, restated, up to the numpy resampling; then the rule with the same uniforms
    seeded(4)
    random.random()
    for _ in range(2):
        torch.empty(B, device=DEV).uniform_()
    rand_a, rand_b = np.random.permutation(B), np.random.permutation(B)
    draws = [torch.empty(s, dtype=torch.float32, device=DEV).uniform_(lo, hi) for s, lo, hi in
             ((B, 0, 1), (B, -180, 180), (B, *ELEV), (B, *DIST), ((B, 2), -0.5, 0.5), ((B, 1, 1, 1), 0, 1), ((B, 1, 1), 0, 1), ((B, 1), 0, 1))]
    u = torch.empty((2, B), dtype=torch.float32, device=DEV).uniform_(0.0, 1.0, generator=torch.Generator(device=DEV).manual_seed(99))
    ia, ib, n_bad = resample_np(Ae["delta_vertices"].cpu().numpy(), rand_a, rand_b, u.cpu().numpy())
    assert n_bad == len(collapsed) and not np.isin(ia, collapsed).any() and not np.isin(ib, collapsed).any()
    ref = eager(Ae, torch.from_numpy(ia).to(DEV), torch.from_numpy(ib).to(DEV), draws[6], draws[5], draws[7])
    for k in KEYS:
        assert torch.equal(Ai[k], ref[k]), k
    assert torch.equal(Ai["azimuths"], -draws[1])


def test_no_host_sync():
    B, o = 48, opt()
    Ae = full_attrs(B, seed=13)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            block(Ae, o, B)
            raised = False
        except RuntimeError:
            raised = True
        if not raised:
            pytest.skip("this torch build does not raise on a synchronising call under set_sync_debug_mode('error')")
        Ai, Ae90 = IP.interpolate_attributes(Ae, o, ELEV, DIST)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert torch.isfinite(Ai["textures"]).all()


def test_end_to_end_gradients_match_the_eager_block():
    pkg = importlib.import_module("3d-magic-mirror_amd")
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "smpl_uv_642.npz"), 64)
    B = 6
    att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, B, 64, 64, seed=21)
    o = opt(lambda_reg=1.0, lambda_flipz=0.1, lambda_edge=0.0, lambda_depth=0.0, lambda_depthR=0.0, lambda_depthC=0.0, lambda_deform=0.0,
            flipL1=False, temp=1.0, L1=False, chamfer=False, azim=1)
    grads = []
    for use_ours in (True, False):
        leaves = {k: v.to(DEV).requires_grad_() for k, v in att.items() if torch.is_tensor(v)}
        Ae = dict(leaves)
        _, Ae = dr.render(no_mask=True, **Ae)
        seeded(8)
        if use_ours:
            Ai, _ = IP.interpolate_attributes(Ae, o, ELEV, DIST)
        else:
            Ai, _, _ = block(Ae, o, B)
        rgbs, Ai = dr.render(no_mask=True, **Ai)
        loss = dr.recon_data(rgbs, gt.to(DEV), no_mask=True)
        reg, flip, _ = dr.regularization(Ae, Ai, Ai, o)
        (loss + reg + flip).backward()
        grads.append({k: v.grad for k, v in leaves.items() if v.grad is not None})
    assert set(grads[0]) == set(grads[1]) and {"vertices", "textures", "lights", "bg", "delta_vertices"} <= set(grads[0])
    for k in grads[0]:
        grad_close(grads[0][k], grads[1][k], rtol=1e-4, what=k)
