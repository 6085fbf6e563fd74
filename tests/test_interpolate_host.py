"""Attribute interpolation (3d-magic-mirror_amd/interpolate.py, csrc/mm_interp.hip) without a GPU: the C ABI's mirror and argument
checks, the Python API's validation, and the numpy restatement of the collapse-resampling rule that tests/test_gpu_interpolate.py
measures the kernel against."""
import ctypes
import importlib
import types

import numpy as np
import pytest
import torch

IP = importlib.import_module("3d-magic-mirror_amd.interpolate")
N = importlib.import_module("3d-magic-mirror_amd._native")


# ---- the resampling rule, restated in numpy -------------------------------------------------------------------------------------
def resample_np(delta_vertices, idx_a, idx_b, uniforms, threshold=0.4):
    """(idx_a, idx_b, n_bad): bad[b] = ((|x| + |y|) + |z|) / 3 > threshold over the last vertex, in float32 (NaN is not bad); every
    slot holding a bad sample gets good[min(floor(fl(u * n_good)), n_good - 1)], good ascending; no good sample: unchanged."""
    last = np.abs(np.asarray(delta_vertices, dtype=np.float32)[:, -1, :])
    mean = ((last[:, 0] + last[:, 1]) + last[:, 2]) / np.float32(3)
    with np.errstate(invalid="ignore"):
        bad = mean > np.float32(threshold)
    B = bad.shape[0]
    good = np.flatnonzero(~bad)
    ia, ib = np.array(idx_a, dtype=np.int64), np.array(idx_b, dtype=np.int64)
    if good.size == 0:
        return ia, ib, B
    u = np.asarray(uniforms, dtype=np.float32)
    for which, idx in enumerate((ia, ib)):
        for s in range(B):
            k = idx[s]
            if 0 <= k < B and bad[k]:
                f = u[which, s] * np.float32(good.size)
                m = min(int(np.floor(f)), good.size - 1) if f >= 1 else 0
                idx[s] = good[m]
    return ia, ib, int(bad.sum())


def test_numpy_rule_matches_the_reference_loop_in_distribution():
    """with u drawn uniformly, the rule picks every good sample with the same probability, like np.random.choice(good)"""
    rng = np.random.default_rng(3)
    B = 8
    dv = np.zeros((B, 5, 3), np.float32)
    dv[[1, 4], -1, :] = 1.0                               # samples 1 and 4 collapsed
    counts = np.zeros(B, np.int64)
    for _ in range(2000):
        ia, ib, n_bad = resample_np(dv, rng.permutation(B), rng.permutation(B), rng.random((2, B), dtype=np.float32))
        assert n_bad == 2 and not np.isin(ia, [1, 4]).any() and not np.isin(ib, [1, 4]).any()
        for idx in (ia, ib):
            for s in range(B):
                counts[idx[s]] += 1
    picks = counts - 2 * 2000                            # every good sample appears once per permutation before any redraw
    good = [0, 2, 3, 5, 6, 7]
    assert picks[[1, 4]].tolist() == [-4000, -4000]
    share = picks[good] / picks[good].sum()
    assert np.abs(share - 1 / 6).max() < 0.03, share


def test_numpy_rule_edges():
    B = 4
    dv = np.zeros((B, 2, 3), np.float32)
    ia, ib = np.array([3, 2, 1, 0]), np.array([0, 1, 2, 3])
    u = np.zeros((2, B), np.float32)
    assert [x.tolist() if hasattr(x, "tolist") else x for x in resample_np(dv, ia, ib, u)] == [[3, 2, 1, 0], [0, 1, 2, 3], 0]
    dv[:, -1, 0] = 5.0                                    # every sample bad: unchanged, n_bad = B
    assert resample_np(dv, ia, ib, u)[2] == B and resample_np(dv, ia, ib, u)[0].tolist() == [3, 2, 1, 0]
    dv[:, -1, 0] = np.nan                                 # NaN means are not bad
    assert resample_np(dv, ia, ib, u)[2] == 0
    dv[0, -1, 0] = 5.0                                    # one bad sample; u just below 1 picks the last good one
    u[:] = np.nextafter(np.float32(1), np.float32(0))
    out_a, out_b, n_bad = resample_np(dv, ia, ib, u)
    assert n_bad == 1 and out_a.tolist() == [3, 2, 1, 3] and out_b.tolist() == [3, 1, 2, 3]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_mirrors_the_new_structs_and_symbols(pkg):
    L = N.lib()
    assert N.ABI_VERSION == 9 == L.mm_abi_version()
    for i, cls in zip((24, 25), (N.MMInterpDesc, N.MMInterpGrads)):
        assert L.mm_struct_size(i) == ctypes.sizeof(cls) > 0, cls.__name__
    for name in ("mm_interp_query_workspace", "mm_collapse_resample", "mm_attribute_mix_forward", "mm_attribute_mix_backward"):
        assert name in N.EXPORTS and hasattr(L, name), name


def _desc(B=4, V=10, Ht=8, Wt=8, H=0, W=0):
    d = N.MMInterpDesc()
    d.B, d.V, d.Ht, d.Wt, d.H, d.W = B, V, Ht, Wt, H, W
    return d


def _fill(d, with_bg=False):
    fake = ctypes.c_void_p(16)                            # never dereferenced: every call below must fail validation first
    for f in ("vertices", "delta_vertices", "textures", "lights", "out_vertices", "out_delta_vertices", "out_textures", "out_lights",
              "idx_a", "idx_b", "alpha_shape", "alpha_texture", "alpha_light"):
        setattr(d, f, fake)
    if with_bg:
        d.bg = d.out_bg = fake
    return d


def test_entry_points_reject_bad_arguments_before_any_launch(pkg):
    L = N.lib()
    fake = ctypes.c_void_p(16)
    assert L.mm_attribute_mix_forward(None, None) == -1 and L.mm_attribute_mix_backward(None, None, None) == -1
    assert L.mm_interp_query_workspace(None) == 0
    assert L.mm_attribute_mix_forward(ctypes.byref(N.MMInterpDesc()), None) == -2          # every size 0
    for f in ("B", "V", "Ht", "Wt"):
        d = _fill(_desc())
        setattr(d, f, 0)
        assert L.mm_attribute_mix_forward(ctypes.byref(d), None) == -2, f
        assert L.mm_interp_query_workspace(ctypes.byref(d)) == 0, f
    d = _fill(_desc(), with_bg=True)                                                         # bg given: H and W are checked
    assert L.mm_attribute_mix_forward(ctypes.byref(d), None) == -2
    d = _fill(_desc(B=65536))
    assert L.mm_attribute_mix_forward(ctypes.byref(d), None) == -5
    assert L.mm_interp_query_workspace(ctypes.byref(d)) == 0
    d = _fill(_desc(Ht=1 << 15, Wt=1 << 15))                                                 # a row of 3 * 2^30 floats
    assert L.mm_attribute_mix_forward(ctypes.byref(d), None) == -5
    d = _desc()
    assert L.mm_attribute_mix_forward(ctypes.byref(d), None) == -1                          # shape fine, pointers missing
    d = _fill(_desc())
    d.bg = fake                                                                              # bg without out_bg
    d.H = d.W = 4
    assert L.mm_attribute_mix_forward(ctypes.byref(d), None) == -1
    # backward: pairs, workspace
    d = _fill(_desc())
    ws = L.mm_interp_query_workspace(ctypes.byref(d))
    assert ws > 0 and ws % 256 == 0
    assert L.mm_interp_query_workspace(ctypes.byref(_fill(_desc(B=400)))) > ws
    g = N.MMInterpGrads()
    assert L.mm_attribute_mix_backward(ctypes.byref(d), ctypes.byref(g), None) == 0         # nothing asked: nothing launched
    g.grad_out_textures = fake                                                               # upstream without its destination
    assert L.mm_attribute_mix_backward(ctypes.byref(d), ctypes.byref(g), None) == -1
    g = N.MMInterpGrads()
    g.grad_out_bg = g.grad_bg = fake                                                         # bg's pair: H and W are checked
    assert L.mm_attribute_mix_backward(ctypes.byref(d), ctypes.byref(g), None) == -2
    g = N.MMInterpGrads()
    g.grad_out_lights = g.grad_lights = fake
    assert L.mm_attribute_mix_backward(ctypes.byref(d), ctypes.byref(g), None) == -3        # no workspace
    d.workspace, d.workspace_bytes = fake, ws - 1
    assert L.mm_attribute_mix_backward(ctypes.byref(d), ctypes.byref(g), None) == -3        # short workspace
    d.B = 65536
    assert L.mm_attribute_mix_backward(ctypes.byref(d), ctypes.byref(g), None) == -5
    # the resampling
    p = fake
    assert L.mm_collapse_resample(4, 10, None, p, p, p, 0.4, p, None) == -1
    assert L.mm_collapse_resample(4, 10, p, p, p, p, 0.4, None, None) == -1
    assert L.mm_collapse_resample(0, 10, p, p, p, p, 0.4, p, None) == -2
    assert L.mm_collapse_resample(4, 0, p, p, p, p, 0.4, p, None) == -2
    assert L.mm_collapse_resample(65536, 10, p, p, p, p, 0.4, p, None) == -5
    assert L.mm_last_error_detail().decode() == ""                                           # nothing launched, nothing recorded


# ---- the Python API's validation (all of it before any device work) ----------------------------------------------------------------
def _attrs(B=4, V=6, Ht=4, Wt=8, H=8, W=8, dev="cpu"):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)  # noqa: E731
    return {"vertices": r(B, V, 3), "delta_vertices": r(B, V, 3), "textures": r(B, 3, Ht, Wt), "bg": r(B, 3, H, W), "lights": r(B, 9),
            "azimuths": r(B), "elevations": r(B), "distances": r(B), "biases": r(B, 2)}


def _alphas(B=4):
    return torch.rand(B, 1, 1), torch.rand(B, 1, 1, 1), torch.rand(B, 1)


def test_wrapper_refuses_cpu_tensors(pkg):
    A = _attrs()
    with pytest.raises(RuntimeError, match="device memory"):
        IP.mix_attributes(A, np.arange(4), np.arange(4), *_alphas())
    with pytest.raises(RuntimeError, match="device memory"):
        IP.resample_collapsed(A["delta_vertices"], np.arange(4), np.arange(4), torch.rand(2, 4))


def test_host_indices_are_checked(pkg):
    dev = torch.device("cuda:0")
    for bad, msg in (([0, 1, 2, 4], "outside"), ([0, 1, -1, 2], "outside"), ([0, 1, 2], "hold 4"), (np.zeros((2, 2), int), "hold 4"),
                     (np.array([0.0, 1.0, 2.0, 3.0]), "hold 4"), (torch.tensor([0, 1, 2, 7]), "outside")):
        with pytest.raises(ValueError, match=msg):
            IP._indices(bad, 4, dev, "idx_a")


def test_alphas_that_require_grad_and_bad_alphas_are_refused(pkg):
    dev = torch.device("cpu")
    with pytest.raises(RuntimeError, match="requires grad"):
        IP._alpha(torch.rand(4, 1, 1, requires_grad=True), 4, dev, "alpha_shape")
    with pytest.raises(ValueError, match="shape"):
        IP._alpha(torch.rand(4, 2), 4, dev, "alpha_light")
    with pytest.raises(ValueError, match="float32"):
        IP._alpha(torch.rand(4, 1, dtype=torch.float64), 4, dev, "alpha_light")
    assert IP._alpha(torch.rand(4, 1, 1, 1), 4, dev, "alpha_texture").shape == (4,)


def test_sources_are_checked_and_upcast(pkg):
    dev = torch.device("cpu")
    A = _attrs()
    with pytest.raises(ValueError, match="shape"):
        IP._source(A, "lights", (4, 8), dev)
    A["lights"] = A["lights"].to(torch.int32)
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        IP._source(A, "lights", (4, 9), dev)
    A["bg"] = A["bg"].half().transpose(2, 3)
    t = IP._source(A, "bg", (4, 3, 8, 8), dev)
    assert t.dtype == torch.float32 and t.is_contiguous() and torch.equal(t, A["bg"].float())


def _opt(**kw):
    o = dict(hard=True, hard_range=20, inv=0, lambda_ic=0.1, azi_scope=360, bias_range=0.5, beta=0.0, bg=True)
    o.update(kw)
    return types.SimpleNamespace(**o)


def test_beta_raises_like_the_reference(pkg):
    with pytest.raises(RuntimeError, match="legacy constructor"):
        IP.interpolate_attributes(_attrs(), _opt(beta=0.5), (0, 30), (2, 3))
    # without the interpolation the reference never reaches that line: only the device check stops this CPU call
    with pytest.raises(RuntimeError, match="device memory"):
        IP.interpolate_attributes(_attrs(), _opt(beta=0.5, lambda_ic=0.0), (0, 30), (2, 3))
