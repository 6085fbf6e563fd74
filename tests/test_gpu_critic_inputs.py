"""Critic inputs on the MI355X (csrc/mm_critic.hip) against the eager fp32 torch restatement of the block evaluated on the CPU
(tests/test_critic_inputs_host.py: restate), bit for bit where the operations are the same, and against the float64 form of the
backward within a derived bound where the summation differs (the alpha plane's gradient under unmask 0)."""
import importlib
import itertools
import os

import pytest
import torch
import torch.nn as nn

from conftest import TEMPLATES
from parity_bar import grad_close
from test_critic_inputs_host import alpha_bound, backward64, backward_rgb32, channel_map, restate

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CI = importlib.import_module("3d-magic-mirror_amd.critic_inputs")
SHAPES = [(48, 128, 128), (48, 128, 64), (3, 5, 7), (1, 8, 8)]          # (3,5,7): H*W % 4 != 0, the one-pixel-per-lane path


def images(B, H, W, seed, layouts=(1, 1, 1)):
    """three (B,4,H,W) CPU images, colour in [-1, 2), alpha in [0, 1] with exact 0s and 1s; layouts[i] = 1: NHWC-dense memory"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for nhwc in layouts:
        x = torch.rand(B, H, W, 4, generator=g)
        x[..., :3] = x[..., :3] * 3 - 1
        a = x[..., 3] * 1.5 - 0.25
        x[..., 3] = a.clamp(0, 1)
        out.append(x.permute(0, 3, 1, 2) if nhwc else x.permute(0, 3, 1, 2).contiguous())
    return out


def to_dev(x):
    """the same values with the same strides in device memory"""
    d = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=DEV)
    d.copy_(x)
    return d


def alphas(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, generator=g), torch.rand(B, 1, 1, 1, generator=g)


def check_forward(xs, unmask, al):
    ci = CI.critic_inputs(*[to_dev(x) for x in xs], unmask=unmask, gp_alphas=None if al is None else tuple(a.to(DEV) for a in al), gp=al is not None)
    d, g, gp1, gp2 = restate(*xs, unmask, al)
    B = xs[0].shape[0]
    assert ci.d_batch.is_contiguous() and ci.g_batch.is_contiguous() and ci.d_batch.shape == d.shape and ci.g_batch.shape == g.shape
    assert torch.equal(ci.d_batch.cpu(), d), "d_batch"
    assert torch.equal(ci.g_batch.cpu(), g), "g_batch"
    assert ci.g_batch.data_ptr() == ci.d_batch[B:].data_ptr()
    if al is None:
        assert ci.gp_er90 is None and ci.gp_ir is None and ci.alphas is None
    else:
        assert torch.equal(ci.gp_er90.cpu(), gp1), "gp_er90"
        assert torch.equal(ci.gp_ir.cpu(), gp2), "gp_ir"
        assert ci.gp_er90.is_leaf and ci.gp_er90.requires_grad and ci.gp_ir.is_leaf and ci.gp_ir.requires_grad and ci.gp_er90.is_contiguous()
        assert torch.equal(ci.alphas[0].cpu(), al[0].reshape(B)) and torch.equal(ci.alphas[1].cpu(), al[1].reshape(B))
    return ci


# ---- forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unmask", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_is_the_eager_composition_bit_for_bit(shape, unmask):
    B, H, W = shape
    check_forward(images(B, H, W, seed=B + unmask), unmask, alphas(B, seed=7))
    check_forward(images(B, H, W, seed=B + unmask + 10, layouts=(0, 1, 0)), unmask, None)


@pytest.mark.parametrize("layouts", list(itertools.product((0, 1), repeat=3)))
def test_every_layout_combination(layouts):
    for unmask in (0, 1, 2):
        check_forward(images(5, 12, 20, seed=3, layouts=layouts), unmask, alphas(5, seed=2))


def test_alphas_of_exactly_zero_and_one():
    B = 4
    xs = images(B, 16, 8, seed=9)
    a1 = torch.tensor([0.0, 1.0, 0.0, 1.0])
    a2 = torch.tensor([1.0, 1.0, 0.0, 0.5])
    for unmask in (0, 1, 2):
        ci = check_forward(xs, unmask, (a1, a2))
        Ma, M1 = channel_map(xs[0], unmask), channel_map(xs[1], unmask)
        assert torch.equal(ci.gp_er90[0].cpu(), M1[0]) and torch.equal(ci.gp_er90[1].cpu(), Ma[1])   # 0: the fake (+0 * real is exact); 1: the real image


def test_other_strides_and_dtypes_are_converted():
    B, H, W = 2, 8, 12
    xs = images(B, H, W, seed=5, layouts=(0, 0, 0))
    wide = torch.zeros(B, 4, H, 2 * W)
    wide[..., ::2] = xs[1]
    odd = to_dev(wide)[..., ::2]                                         # neither layout: copied
    half = xs[2].half()
    ci = CI.critic_inputs(to_dev(xs[0]).double(), odd, to_dev(half), unmask=0, gp=False)
    d, _, _, _ = restate(xs[0], xs[1], half.float(), 0)
    assert torch.equal(ci.d_batch.cpu(), d)


def test_drawn_alphas_come_from_the_generator():
    B = 6
    xs = [to_dev(x) for x in images(B, 8, 8, seed=1)]
    g = torch.Generator(device=DEV).manual_seed(5)
    ci = CI.critic_inputs(*xs, unmask=1, generator=g)
    ref = torch.rand((2, B), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(ci.alphas[0], ref[0]) and torch.equal(ci.alphas[1], ref[1])
    assert float(ref.min()) >= 0.0 and float(ref.max()) < 1.0
    _, _, gp1, gp2 = restate(*[x.cpu() for x in xs], 1, (ref[0].cpu(), ref[1].cpu()))
    assert torch.equal(ci.gp_er90.cpu(), gp1) and torch.equal(ci.gp_ir.cpu(), gp2)


# ---- storage ----------------------------------------------------------------------------------------------------------------------
def test_storage_and_requires_grad():
    B = 3
    xa, x1, x2 = (to_dev(x) for x in images(B, 8, 8, seed=2))
    ci = CI.critic_inputs(xa, x1, x2, gp=False)
    assert ci.g_batch.data_ptr() == ci.d_batch[B:].data_ptr() and not ci.d_batch.requires_grad and not ci.g_batch.requires_grad
    for r1, r2 in ((True, False), (False, True), (True, True)):
        ci = CI.critic_inputs(xa.clone().requires_grad_(), x1.clone().requires_grad_(r1), x2.clone().requires_grad_(r2), gp=False)
        assert ci.g_batch.data_ptr() == ci.d_batch[B:].data_ptr() and not ci.d_batch.requires_grad and ci.g_batch.requires_grad
    ci = CI.critic_inputs(xa.clone().requires_grad_(), x1, x2, gp=False)           # only the real image: nothing to differentiate
    assert not ci.g_batch.requires_grad


# ---- backward ---------------------------------------------------------------------------------------------------------------------
def run_backward(xs, unmask, g, need=(True, True)):
    xa = to_dev(xs[0]).requires_grad_()
    x1, x2 = to_dev(xs[1]).requires_grad_(need[0]), to_dev(xs[2]).requires_grad_(need[1])
    ci = CI.critic_inputs(xa, x1, x2, unmask=unmask, gp=False)
    (ci.g_batch * g.to(DEV)).sum().backward()
    assert xa.grad is None
    return x1, x2


@pytest.mark.parametrize("unmask", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("layouts", [(1, 1, 1), (0, 0, 1)])
def test_backward(shape, unmask, layouts):
    B, H, W = shape
    C = 4 if unmask == 2 else 3
    xs = images(B, H, W, seed=20 + unmask, layouts=layouts)
    g = torch.randn(2 * B, C, H, W, generator=torch.Generator().manual_seed(31))
    x1, x2 = run_backward(xs, unmask, g)
    for j, xd in enumerate((x1, x2)):
        x, gj, got = xs[1 + j], g[j * B:(j + 1) * B], xd.grad
        assert got.stride() == xd.stride() == x.stride(), (got.stride(), x.stride())
        got = got.cpu()
        assert torch.equal(got[:, :3], backward_rgb32(x, gj, unmask)), "colour planes, fake %d" % j
        if unmask == 1:
            assert (got[:, 3] == 0).all()
        elif unmask == 2:
            assert torch.equal(got[:, 3], gj[:, 3])
        else:
            r64 = backward64(x, gj, 0)[:, 3]
            err, bound = (got[:, 3].double() - r64).abs(), alpha_bound(x, gj)
            print("unmask 0 alpha plane, fake %d: max err %.3e, max err / bound %.3f" % (j, float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
            assert (err <= bound).all()
    y1, y2 = run_backward(xs, unmask, g)                                  # two runs agree to the bit
    assert torch.equal(x1.grad, y1.grad) and torch.equal(x2.grad, y2.grad)


def test_backward_for_one_fake_only_and_without_upstream():
    B, H, W = 4, 16, 16
    xs = images(B, H, W, seed=40)
    g = torch.randn(2 * B, 3, H, W, generator=torch.Generator().manual_seed(41))
    full = run_backward(xs, 0, g)
    for need in ((True, False), (False, True)):
        x1, x2 = run_backward(xs, 0, g, need)
        for k, (x, f) in enumerate(zip((x1, x2), full)):
            assert (x.grad is None) if not need[k] else torch.equal(x.grad, f.grad)
    x1 = to_dev(xs[1]).requires_grad_()
    ci = CI.critic_inputs(to_dev(xs[0]), x1, to_dev(xs[2]), gp=False)
    (ci.g_batch.sum() * 0 + x1.sum()).backward()                          # a zero upstream still runs; a result nobody uses does not
    assert x1.grad is not None
    x1.grad = None
    CI.critic_inputs(to_dev(xs[0]), x1, to_dev(xs[2]), gp=False)
    assert x1.grad is None


@pytest.mark.parametrize("unmask", [0, 1, 2])
def test_the_same_tensor_as_both_fakes_gets_the_sum(unmask):
    B, H, W = 4, 16, 24
    C = 4 if unmask == 2 else 3
    xs = images(B, H, W, seed=50)
    g = torch.randn(2 * B, C, H, W, generator=torch.Generator().manual_seed(51))
    a, b = run_backward([xs[0], xs[1], xs[1]], unmask, g)
    x = to_dev(xs[1]).requires_grad_()
    ci = CI.critic_inputs(to_dev(xs[0]), x, x, unmask=unmask, gp=False)
    assert torch.equal(ci.g_batch[:B], ci.g_batch[B:])
    (ci.g_batch * g.to(DEV)).sum().backward()
    assert torch.equal(x.grad, a.grad + b.grad)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def small_critic(cin, seed=0):
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Conv2d(cin, 16, 4, 2, 1), nn.LeakyReLU(0.2), nn.Conv2d(16, 1, 4, 2, 1)).to(DEV)
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def test_end_to_end_render_critic_backward():
    """render x2 -> critic_inputs(unmask 0) -> conv critic -> backward, against the same chain from eager ops; a render's gradient
    arrives with the render's own NHWC strides"""
    pkg = importlib.import_module("3d-magic-mirror_amd")
    B, S = 4, 64
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), S)
    atts = [pkg.synthetic.synthetic_batch(dr.vertices_init, B, S, S, seed=s)[0] for s in (61, 62)]
    xa = torch.rand(B, 4, S, S, generator=torch.Generator().manual_seed(63)).to(DEV)
    critic = small_critic(3)
    names = ("vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases")
    torch.backends.cudnn.deterministic = True
    runs = []
    for fused in (True, False):
        sets = [{k: (v.to(DEV).requires_grad_(k in names) if torch.is_tensor(v) else v) for k, v in a.items()} for a in atts]
        x1, _ = dr.render(no_mask=True, **sets[0])
        x2, _ = dr.render(no_mask=True, **sets[1])
        assert x1.stride() == (4 * S * S, 1, 4 * S, 4)
        seen = []
        if fused:
            x1.register_hook(lambda gr: seen.append((gr.stride(), gr.permute(0, 2, 3, 1).is_contiguous())))   # the gradient as the render's node gets it
            batch = CI.critic_inputs(xa, x1, x2, unmask=0, gp=False).g_batch
        else:
            batch = restate(xa, x1, x2, 0)[1]
            assert torch.equal(batch, fused_batch)
            # cat keeps the renders' channels-last memory format, and MIOpen's channels-last convolution rounds differently from its NCHW
            # one (the same values fed in either layout: outputs 1-2 ulp apart).  The scalar below compares the two chains, not two
            # convolution algorithms: the eager batch is fed in the layout critic_inputs returns.  .contiguous() changes no value.
            batch = batch.contiguous()
        fused_batch = batch.detach()
        out = critic(batch).mean()
        out.backward()
        if fused:
            assert seen == [(x1.stride(), True)], seen
        runs.append((out.detach(), [{k: s[k].grad for k in names} for s in sets]))
    print("critic output fused %r eager %r" % (float(runs[0][0]), float(runs[1][0])))
    for r in (0, 1):
        for k in names:
            assert runs[0][1][r][k] is not None and runs[1][1][r][k] is not None, k
            grad_close(runs[0][1][r][k], runs[1][1][r][k], rtol=1e-4, what="render %d %s" % (r, k))
    assert torch.equal(runs[0][0], runs[1][0]), (float(runs[0][0]), float(runs[1][0]))


def test_trainer_step_with_fused_critic_is_the_step():
    mod = importlib.import_module("3d-magic-mirror_amd.trainer_step")
    path = os.path.join(TEMPLATES, "sphere.npz")
    torch.backends.cudnn.deterministic = True
    runs = []
    for fused in (True, False):
        ts = mod.TrainerStep(path, 64, 4, DEV, fused_critic=fused)
        ts.step(optimize=False)
        runs.append((ts.last["fake"].clone(), [p.grad.detach().clone() for p in ts.netE.parameters()]))
    print("fake fused %r eager %r" % (float(runs[0][0]), float(runs[1][0])))
    for i, (a, b) in enumerate(zip(runs[0][1], runs[1][1])):
        grad_close(a, b, rtol=1e-4, what="netE parameter %d" % i)
    assert torch.equal(runs[0][0], runs[1][0]), (float(runs[0][0]), float(runs[1][0]))
