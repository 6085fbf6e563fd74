"""Critic inputs (3d-magic-mirror_amd/critic_inputs.py, csrc/mm_critic.hip) without a GPU: the C ABI's mirror and argument checks, the
Python API's validation, a static check of the kernels' ISA (16-byte accesses only, no scratch, no spills in the vector
instantiations), and the eager torch restatement of the block -- with a float64 form of its backward -- that
tests/test_gpu_critic_inputs.py measures the kernels against."""
import ctypes
import importlib
import os
import re
import subprocess
import tempfile

import pytest
import torch

CI = importlib.import_module("3d-magic-mirror_amd.critic_inputs")
N = importlib.import_module("3d-magic-mirror_amd._native")


# ---- the block, restated in eager torch (any device, any float dtype) ---------------------------------------------------------------
def channel_map(X, unmask):
    """M(X): 0 -> the image over white with its own alpha, 1 -> the colour planes, 2 -> all four planes"""
    if unmask == 0:
        rgb, m = X[:, :3], X[:, 3:4]
        return rgb * m + torch.ones_like(rgb) * (1 - m)
    return X[:, :3] if unmask == 1 else X


def restate(Xa, Xer90, Xir, unmask, alphas=None):
    """(d_batch, g_batch, gp_er90, gp_ir) as eager torch composes them: three maps, detached copies and a cat for the D step, a cat of
    the two fakes for the G step, and the two interpolates a * real + ((1 - a) * fake) with a of shape (B,1,1,1)"""
    Ma, M1, M2 = channel_map(Xa, unmask), channel_map(Xer90, unmask), channel_map(Xir, unmask)
    d_batch = torch.cat((Ma.detach().clone(), M1.detach().clone(), M2.detach().clone()), 0)
    g_batch = torch.cat((M1, M2), 0)
    gp1 = gp2 = None
    if alphas is not None:
        a1, a2 = (a.reshape(-1, 1, 1, 1) for a in alphas)
        gp1 = a1 * Ma.detach() + ((1 - a1) * M1.detach())
        gp2 = a2 * Ma.detach() + ((1 - a2) * M2.detach())
    return d_batch, g_batch, gp1, gp2


def backward_rgb32(X, g, unmask):
    """the colour planes of the gradient of sum(g * M(X)) w.r.t. X, as fp32 torch rounds them: g * m, or g"""
    return g[:, :3] * X[:, 3:4] if unmask == 0 else g[:, :3].clone()


def backward64(X, g, unmask):
    """the gradient of sum(g * M(X)) w.r.t. X (B,4,H,W) in float64"""
    X, g = X.double(), g.double()
    out = torch.zeros_like(X)
    if unmask == 0:
        out[:, :3] = g * X[:, 3:4]
        out[:, 3] = (g * (X[:, :3] - 1.0)).sum(1)
    elif unmask == 1:
        out[:, :3] = g
    else:
        out.copy_(g)
    return out


def alpha_bound(X, g):
    """unmask 0: |d m - float64| <= 8 * 2^-24 * sum_c |g_c| * (|rgb_c| + 1) -- per term the subtraction and the product round once each
    (relative 2^-24 each, on a term of at most |g_c| (|rgb_c| + 1)), the two adds once each on partial sums no larger than the sum of
    the terms: under 4 * 2^-24 of that sum in all, and a factor of two to spare"""
    return 8.0 * 2.0 ** -24 * (g.double().abs() * (X[:, :3].double().abs() + 1.0)).sum(1)


def test_restatement_agrees_with_autograd_and_float64():
    g0 = torch.Generator().manual_seed(4)
    X = torch.rand(3, 4, 5, 7, generator=g0)
    X[:, :3] = X[:, :3] * 3 - 1
    for unmask in (0, 1, 2):
        C = 4 if unmask == 2 else 3
        g = torch.randn(3, C, 5, 7, generator=g0)
        Xl = X.clone().requires_grad_()
        (channel_map(Xl, unmask) * g).sum().backward()
        r64 = backward64(X, g, unmask)
        assert torch.equal(Xl.grad[:, :3], backward_rgb32(X, g, unmask))
        assert (Xl.grad.double() - r64).abs().max() < 1e-5
        if unmask == 0:
            assert ((Xl.grad[:, 3].double() - r64[:, 3]).abs() <= alpha_bound(X, g)).all()
    d, gb, gp1, gp2 = restate(X, X + 1, X + 2, 0, (torch.zeros(3), torch.ones(3)))
    assert d.shape == (9, 3, 5, 7) and gb.shape == (6, 3, 5, 7) and torch.equal(d[3:], gb)
    assert torch.equal(gp1, channel_map(X + 1, 0)) and torch.equal(gp2, channel_map(X, 0))      # alpha 0: the fake; alpha 1: the real image


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_mirrors_the_new_structs_and_symbols(pkg):
    L = N.lib()
    assert N.ABI_VERSION == 9 == L.mm_abi_version()
    for i, cls in zip((27, 28), (N.MMCriticDesc, N.MMCriticGrads)):
        assert L.mm_struct_size(i) == ctypes.sizeof(cls) > 0, cls.__name__
    for name in ("mm_critic_inputs_forward", "mm_critic_inputs_backward"):
        assert name in N.EXPORTS and hasattr(L, name), name


FAKE = ctypes.c_void_p(16)                                # never dereferenced: every call below must fail validation first


def _desc(B=4, H=8, W=8, unmask=0, gp=True):
    d = N.MMCriticDesc()
    d.B, d.H, d.W, d.unmask = B, H, W, unmask
    d.Xa = d.Xer90 = d.Xir = d.out_batch = FAKE
    if gp:
        d.alpha_er90 = d.alpha_ir = d.out_gp_er90 = d.out_gp_ir = FAKE
    return d


def test_entry_points_reject_bad_arguments_before_any_launch(pkg):
    L = N.lib()
    fwd = lambda d: L.mm_critic_inputs_forward(ctypes.byref(d), None)  # noqa: E731
    assert L.mm_critic_inputs_forward(None, None) == -1 and L.mm_critic_inputs_backward(None, None, None) == -1
    assert L.mm_critic_inputs_backward(ctypes.byref(_desc()), None, None) == -1
    assert fwd(N.MMCriticDesc()) == -2                                                        # every size 0
    for f in ("B", "H", "W"):
        for v in (0, -3):
            d = _desc()
            setattr(d, f, v)
            assert fwd(d) == -2, (f, v)
            assert L.mm_critic_inputs_backward(ctypes.byref(d), ctypes.byref(N.MMCriticGrads()), None) == -2, (f, v)
    for um in (-1, 3):
        assert fwd(_desc(unmask=um)) == -2, um
    for lone in ("alpha_er90", "alpha_ir"):                                                    # one alpha without the other
        d = _desc(gp=False)
        setattr(d, lone, FAKE)
        assert fwd(d) == -2, lone
    for f in ("Xa", "Xer90", "Xir", "out_batch", "out_gp_er90", "out_gp_ir"):
        d = _desc()
        setattr(d, f, None)
        assert fwd(d) == -1, f
    assert fwd(_desc(B=1 << 20, H=1 << 12, W=1 << 12)) == -5                                    # the chunk count leaves an int32
    # backward
    d, g = _desc(gp=False), N.MMCriticGrads()
    assert L.mm_critic_inputs_backward(ctypes.byref(d), ctypes.byref(g), None) == 0           # no gradient wanted: nothing launched
    g.grad_er90 = FAKE
    assert L.mm_critic_inputs_backward(ctypes.byref(d), ctypes.byref(g), None) == -1          # no upstream gradient
    g.g_batch = FAKE
    d.Xer90 = None
    assert L.mm_critic_inputs_backward(ctypes.byref(d), ctypes.byref(g), None) == -1          # unmask 0 reads the fake
    d.unmask = 4
    assert L.mm_critic_inputs_backward(ctypes.byref(d), ctypes.byref(g), None) == -2
    assert L.mm_last_error_detail().decode() == ""                                             # nothing launched, nothing recorded


# ---- the Python API's validation (all of it before any device work) ----------------------------------------------------------------
def _x(B=2, H=4, W=4, **kw):
    return torch.rand(B, 4, H, W, **kw)


def test_wrapper_validates_before_anything_reaches_a_kernel(pkg):
    x = _x()
    with pytest.raises(RuntimeError, match="device memory"):
        CI.critic_inputs(x, x, x)
    with pytest.raises(ValueError, match=r"shape \(B,4,H,W\)"):
        CI.critic_inputs(x[:, :3], x, x)
    with pytest.raises(ValueError, match=r"shape \(B,4,H,W\)"):
        CI.critic_inputs(x[0], x, x)
    with pytest.raises(ValueError, match="Xir has shape"):
        CI.critic_inputs(x, x, _x(H=8))
    with pytest.raises(ValueError, match="Xer90 has shape"):
        CI.critic_inputs(x, _x(B=3), x)
    with pytest.raises(ValueError, match="float tensor"):
        CI.critic_inputs(x, x.to(torch.int32), x)
    with pytest.raises(ValueError, match="float tensor"):
        CI.critic_inputs(x, x.numpy(), x)
    with pytest.raises(ValueError, match="Xir is on meta"):
        CI.critic_inputs(x, x, _x(device="meta"))
    for um in (3, -1, None):
        with pytest.raises(ValueError, match="unmask"):
            CI.critic_inputs(x, x, x, unmask=um)
    a = torch.rand(2)
    with pytest.raises(RuntimeError, match="requires grad"):
        CI.critic_inputs(x, x, x, gp_alphas=(a, torch.rand(2, requires_grad=True)))
    with pytest.raises(ValueError, match="shape"):
        CI.critic_inputs(x, x, x, gp_alphas=(torch.rand(3), a))
    with pytest.raises(ValueError, match="shape"):
        CI.critic_inputs(x, x, x, gp_alphas=(a, torch.rand(2, 2)))
    with pytest.raises(ValueError, match="float32"):
        CI.critic_inputs(x, x, x, gp_alphas=(a.double(), a))
    with pytest.raises(ValueError, match="pair"):
        CI.critic_inputs(x, x, x, gp_alphas=(a,))
    with pytest.raises(RuntimeError, match="device memory"):                                    # well-formed (B,1,1,1) alphas: only the device check is left
        CI.critic_inputs(x, x, x, gp_alphas=(a.reshape(2, 1, 1, 1), a))


def test_layout_choice(pkg):
    nchw = _x()
    nhwc = torch.rand(2, 4, 4, 4).permute(0, 3, 1, 2)
    t, f = CI._layout(nchw)
    assert t is nchw and f == 0
    t, f = CI._layout(nhwc)
    assert t is nhwc and f == 1 and t.stride() == (64, 1, 16, 4)
    odd = torch.rand(2, 4, 4, 8)[..., ::2]
    t, f = CI._layout(odd)
    assert f == 0 and t.is_contiguous() and torch.equal(t, odd)


def test_package_exports(pkg):
    assert pkg.critic_inputs is CI.critic_inputs and pkg.CriticInputs is CI.CriticInputs
    assert CI.CriticInputs._fields == ("d_batch", "g_batch", "gp_er90", "gp_ir", "alphas")
    mod = importlib.import_module("3d-magic-mirror_amd.trainer_step")
    import inspect
    assert inspect.signature(mod.TrainerStep.__init__).parameters["fused_critic"].default is False


# ---- the kernels' ISA ---------------------------------------------------------------------------------------------------------------
def _kernels(asm):
    """{mangled name: (instructions, metadata text)} of every kernel in a gfx950 assembly file"""
    lines = asm.splitlines()
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN2mm\w*critic_(?:fwd|bwd)_kernel\w*):", l)
        if not m:
            continue
        end = next(k for k in range(i, len(lines)) if "s_endpgm" in lines[k])
        body = [x.split(";")[0].strip() for x in lines[i + 1:end]]
        out[m.group(1)] = [x for x in body if x and not x.endswith(":") and not x.startswith(".")]
    meta = {}
    for entry in re.split(r"\n  - (?=\.)", asm[asm.index("amdhsa.kernels:"):]):                 # one list item per kernel
        m = re.search(r"^\s+\.name:\s+(\S+)$", entry, flags=re.M)
        if m:
            meta[m.group(1)] = entry
    return out, meta


def test_vector_instantiations_move_16_bytes_and_use_no_scratch():
    bn = importlib.import_module("3d-magic-mirror_amd.build_native")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert bn.SOURCES["mm_critic.hip"] == bn.EXACT and "-munsafe-fp-atomics" not in bn.SOURCES["mm_critic.hip"]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "critic.s")
        subprocess.check_call([hipcc] + bn.FLAGS + bn.SOURCES["mm_critic.hip"] + ["-S", "--cuda-device-only", "-o", path,
                                                                                 os.path.join(bn.CSRC, "mm_critic.hip")], stderr=subprocess.DEVNULL)
        asm = open(path).read()
    kernels, meta = _kernels(asm)
    vec = {k: v for k, v in kernels.items() if re.search(r"kernelILi[012]ELi4EE", k)}
    assert len(vec) == 6 and len(kernels) == 12, sorted(kernels)                                # {fwd, bwd} x unmask {0, 1, 2} x {4, 1} pixels per lane
    for name, body in vec.items():
        mem = [x.split()[0] for x in body if re.match(r"(global|flat|buffer|scratch)_", x)]
        loads = [x for x in mem if "load" in x]
        stores = [x for x in mem if "store" in x]
        assert loads and stores, name
        assert set(loads) == {"global_load_dwordx4"}, (name, sorted(set(loads)))
        assert set(stores) == {"global_store_dwordx4"}, (name, sorted(set(stores)))
        assert not any("atomic" in x for x in mem), name
        md = meta[name]
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", md).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s*(\d+)", md).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", md).group(1)) == 0, name
        assert int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", md).group(1)) == 0, name   # no LDS either
