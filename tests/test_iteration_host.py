"""The yardstick of tests/test_gpu_iteration.py, checked against itself on the CPU: the restated iteration (tests/iteration_ref.py) at
the GPU test's cases, with draws from a CPU generator.  It shows that the GPU test would notice what it is meant to notice:

  * the two permutations of every case are non-trivial and differ, and every render shows something;
  * the fp32 restatement holds the GPU test's bar (1e-4 of each gradient's own maximum, face_idx exact) against the float64 one for every
    leaf of every case -- so the device never needs the conditioning escape of parity_bar.grad_close;
  * every loss term, switched off, and every wiring fault of iteration_ref.FAULTS, committed, moves some leaf's float64 gradient by more
    than TEN times that bar;
  * which leaves the reference leaves without gradient."""
import copy

import numpy as np
import pytest
import torch

import iteration_ref as I
from parity_bar import rel_errors

BAR = 1e-4                      # the GPU test's bar on a gradient, relative to the gradient's own maximum
SEEN = 10 * BAR                 # what a switched-off term or a fault must move some leaf's gradient by

REFS = {}
for _name, _case in I.CASES.items():
    REFS.setdefault(I.reference_key(_case), _name)
NAMES = sorted(REFS.values())   # one case per distinct question to the reference (lean / many / fused_critic ask the same one)
_cache = {}


def _setup(name):
    """The case on the CPU: built once and shared, with its fp32 and float64 restatements; nothing in it is modified afterwards."""
    if name not in _cache:
        case = I.CASES[name]
        ts, host, E, R, gt = I.build(case, torch.device("cpu"))
        d = ts.draws()
        run = lambda dtype, opt=None, fault=None: I.iteration_restated(host, E, R, d, opt or ts.opt, I.cpu_critic(ts, dtype), gt, dtype,
                                                                        ts.opt.hard, ts.opt.bg, fault=fault)
        _cache[name] = (case, ts, d, run, run(torch.float32), run(torch.float64))
    return _cache[name]


def test_every_case_of_the_table_is_covered():
    assert set(I.reference_key(c) for c in I.CASES.values()) == set(REFS)
    assert len(NAMES) >= 7


@pytest.mark.parametrize("name", NAMES)
def test_permutations_are_non_trivial_and_every_render_shows_something(name):
    case, ts, d, run, r32, r64 = _setup(name)
    ident = torch.arange(case.B)
    if case.B == 2:
        # adapted: two elements have ONE non-trivial permutation, so the two cannot both be non-trivial and differ; the case asks that
        # the swap occurs (Ai then reads the other sample's attributes)
        assert not torch.equal(d["ra"], ident) or not torch.equal(d["rb"], ident), (d["ra"], d["rb"])
    else:
        assert not torch.equal(d["ra"], ident) and not torch.equal(d["rb"], ident) and not torch.equal(d["ra"], d["rb"]), (d["ra"], d["rb"])
    for i, f in enumerate(r64.face_idx):
        assert (f >= 0).mean() > 0.03, (name, "render #%d" % (i + 1), float((f >= 0).mean()))


@pytest.mark.parametrize("name", NAMES)
def test_fp32_restatement_holds_the_bar_against_float64(name):
    case, ts, d, run, r32, r64 = _setup(name)
    for a, b in zip(r32.face_idx, r64.face_idx):
        assert np.array_equal(a, b), int((a != b).sum())
    for t in I.TERMS:
        assert abs(r32.losses[t] - r64.losses[t]) <= 3e-5 * max(1.0, abs(r64.losses[t])), (t, r32.losses[t], r64.losses[t])
    worst = {}
    for s in ("E", "R"):
        for k in I.LEAVES:
            g32, g64 = r32.grads[s][k], r64.grads[s][k]
            assert (g32 is None) == (g64 is None), (s, k)
            if g64 is None:
                continue
            worst[s, k] = rel_errors(g32, g64)[0]
    print(name, {"%s.%s" % k: "%.1e" % v for k, v in worst.items()})
    assert all(v <= BAR for v in worst.values()), {k: v for k, v in worst.items() if v > BAR}


@pytest.mark.parametrize("name", NAMES)
def test_leaves_without_gradient_are_the_listed_ones(name):
    case, ts, d, run, r32, r64 = _setup(name)
    for r in (r32, r64):
        none = [(s, k) for s in ("E", "R") for k in I.LEAVES if r.grads[s][k] is None or float(np.abs(r.grads[s][k]).max()) == 0.0]
        assert none == I.no_grad_leaves(ts.opt), none


@pytest.mark.parametrize("name", NAMES)
def test_each_term_is_visible(name):
    case, ts, d, run, r32, r64 = _setup(name)
    weights = I.TERM_WEIGHTS + tuple(w for w in I.MESH_WEIGHTS if getattr(ts.opt, w) > 0)
    assert "lambda_deform" in weights and (name != "every_mesh_term" or len(weights) == 9)
    for w in weights:
        opt = copy.copy(ts.opt)
        setattr(opt, w, 0.0)
        e, where = I.moved(run(torch.float64, opt=opt).grads, r64.grads)
        print(name, w, "%.2e" % e, where)
        assert e > SEEN, (w, e, where)


# the cases whose edge a fault does NOT reach: it must change nothing there
UNREACHED = {"shared_image_drops_critic_grad": lambda opt: opt.hard, "ae90_not_a_copy": lambda opt: not opt.hard}


@pytest.mark.parametrize("fault", I.FAULTS)
def test_each_fault_is_caught(fault):
    caught = []
    for name in NAMES:
        case, ts, d, run, r32, r64 = _setup(name)
        if name in ("contour", "contour_ragged") and fault != "recon_on_xir":
            continue                                             # (the contour cases differ from `plain` in recon_data alone)
        bad = run(torch.float64, fault=fault)
        e, where = I.moved(bad.grads, r64.grads)
        print(fault, name, "%.2e" % e, where)
        if fault in UNREACHED and UNREACHED[fault](ts.opt):
            assert e == 0.0 and bad.losses == r64.losses, (name, e)
        elif e > SEEN:
            caught.append(name)
    assert caught, fault
    if fault not in UNREACHED:
        assert len(caught) >= 2, caught                          # (every fault but the two above has its edge in every case)


def test_flipL1_raises_as_the_reference_does():
    case, ts, d, run, r32, r64 = _setup("plain")
    opt = copy.copy(ts.opt)
    opt.flipL1 = True
    with pytest.raises(RuntimeError, match="size of tensor"):
        run(torch.float64, opt=opt)
