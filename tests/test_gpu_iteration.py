"""One generator iteration on the device -- TrainerStep.iteration: four renders in the trainer's dependency order, the critic, recon_data,
the regularisers, ONE backward -- against its restatement from independently pinned pieces on the CPU (tests/iteration_ref.py: the C
oracle's render and recon_data under autograd, reg_oracle.py, brute-force chamfer), in fp32 and float64.  What this holds is the WIRING
between the calls: one attribute tensor feeding several renders, one image feeding two consumers (with hard=False the image whose
recon_data backward is deferred into the render node also carries the critic's gradient), render_many's concatenation and split,
render_geometry standing in for a render, the detached IC target, the per-set packing of the mesh terms.  tests/test_iteration_host.py
shows on the CPU that every such error moves some leaf's gradient by more than ten times the bar used here.

The encoder is out of the picture: set E (what netE(Xa) would return) and set R (what it would return for Xir) are seeded leaf tensors.
Bars, all the project's own: derived attributes bit-equal to the fp32 restatement's; face_idx exact (test_gpu_parity); each loss term
within 3e-5 * max(1, |ref|) (test_regularization_matches_trainer_composition); every leaf gradient within 1e-4 of its own maximum
(parity_bar.grad_close, the float64 restatement deciding a miss: at most one such "cond" per case, printed); leaves the reference leaves
without gradient have None or exact zeros.  Not covered: the stock-PyTorch encoders, Adam, the D update."""
import numpy as np
import pytest
import torch

import iteration_ref as I
from parity_bar import grad_close, rel_errors

pytestmark = pytest.mark.gpu
_refs = {}


def _reference(case, ts, host, E, R, d, gt):
    """The fp32 and float64 restatements for the case's question, computed once and shared by the cases that ask it (same draws)."""
    key = I.reference_key(case)
    if key not in _refs:
        run = lambda dtype: I.iteration_restated(host, E, R, d, ts.opt, I.cpu_critic(ts, dtype), gt, dtype, ts.opt.hard, ts.opt.bg)
        _refs[key] = ({k: v.detach().cpu().clone() for k, v in d.items()}, run(torch.float32), run(torch.float64))
    d0, r32, r64 = _refs[key]
    assert all(torch.equal(d0[k], d[k].cpu()) for k in d0)
    return r32, r64


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_iteration_matches_its_restatement(name):
    case = I.CASES[name]
    dev = torch.device("cuda:0")
    ts, host, E, R, gt = I.build(case, dev)
    Ed = {k: E[k].to(dev).requires_grad_(True) for k in I.LEAVES}
    Rd = {k: R[k].to(dev).requires_grad_(True) for k in I.LEAVES}
    vinit = host.vertices_init.to(dev)
    Ar = I.attributes_of(Rd, vinit)
    asked = []

    def encode(x):
        asked.append((tuple(x.shape), x.requires_grad))
        return dict(Ar)

    face_idx = {}
    render = ts._render

    def recorded(slot, A):
        out = render(slot, A)
        face_idx[slot] = ts.dr.last_face_idx.clone()
        return out
    ts._render = recorded
    d = ts.draws()
    ident = torch.arange(case.B, device=dev)
    if case.B == 2:                                              # (one non-trivial permutation: the swap must occur)
        assert not torch.equal(d["ra"], ident) or not torch.equal(d["rb"], ident)
    else:
        assert not torch.equal(d["ra"], ident) and not torch.equal(d["rb"], ident) and not torch.equal(d["ra"], d["rb"])
    terms = ts.iteration(I.attributes_of(Ed, vinit), encode, draws=d)
    terms["loss"].backward()
    torch.cuda.synchronize()
    assert asked == [((case.B, 4, host.H, host.W), False)]
    r32, r64 = _reference(case, ts, host, E, R, d, gt)

    # derived attributes: single correctly rounded fp32 multiplies, adds and index copies on both sides
    for s in ("Ae90", "Ai", "Aire"):
        if r32.sets[s] is None:
            assert ts.last_sets["Ae90"] is ts.last_sets["Ae"]
            continue
        for k in I.COPIED:
            got, ref = ts.last_sets[s][k], r32.sets[s][k]
            assert (got is None) == (ref is None), (s, k)
            assert got is None or torch.equal(got.detach().cpu(), ref), (s, k, float((got.detach().cpu() - ref).abs().max()))

    # face_idx of every image render
    B = case.B
    if ts.many:
        whole = ts.dr.last_face_idx.cpu().numpy()
        got_idx = {i: whole[i * B:(i + 1) * B] for i in range(3 if ts.opt.hard else 2)}
        assert whole.shape[0] == B * len(got_idx)
    else:
        got_idx = {i: f.cpu().numpy() for i, f in face_idx.items()}
        assert sorted(got_idx) == [0, 1] + ([2] if ts.opt.hard else []) + ([] if ts.lean else [3])
    for slot, ref in zip((0, 1, 2, 3), r32.face_idx):
        if slot in got_idx:
            assert np.array_equal(got_idx[slot], ref), (slot, int((got_idx[slot] != ref).sum()))
            assert (ref >= 0).mean() > 0.03

    # the six loss terms
    for t in I.TERMS:
        diff = abs(float(terms[t].detach()) - r32.losses[t])
        print("ITERATION %s loss %s: device %.8g, fp32 %.8g, float64 %.10g, |device - fp32| %.2e" % (name, t, float(terms[t].detach()), r32.losses[t], r64.losses[t], diff))
    for t in I.TERMS:
        assert abs(float(terms[t].detach()) - r32.losses[t]) <= 3e-5 * max(1.0, abs(r32.losses[t])), (t, float(terms[t].detach()), r32.losses[t])

    # gradients
    none = I.no_grad_leaves(ts.opt)
    verdicts, failures = {}, []
    for s, dev_leaves in (("E", Ed), ("R", Rd)):
        for k in I.LEAVES:
            got = dev_leaves[k].grad
            if (s, k) in none:
                assert r64.grads[s][k] is None or float(np.abs(r64.grads[s][k]).max()) == 0.0
                assert got is None or float(got.abs().max()) == 0.0, (s, k)
                continue
            assert got is not None, (s, k)
            e32, e64 = rel_errors(got, r32.grads[s][k])[0], rel_errors(got, r64.grads[s][k])[0]
            try:
                verdicts[s, k] = grad_close(got, r32.grads[s][k], rtol=1e-4, what="%s, %s.%s" % (name, s, k), ref64=r64.grads[s][k])
            except AssertionError as err:
                verdicts[s, k] = "FAIL"
                failures.append(str(err))
            print("ITERATION %s grad %s.%s: against fp32 %.2e, against float64 %.2e, fp32 against float64 %.2e, max|ref| %.2e: %s"
                  % (name, s, k, e32, e64, rel_errors(r32.grads[s][k], r64.grads[s][k])[0], float(np.abs(r32.grads[s][k]).max()), verdicts[s, k]))
    assert not failures, failures
    cond = [k for k, v in verdicts.items() if v == "cond"]
    assert len(cond) <= 1, cond                                  # (the reference alone needs none: tests/test_iteration_host.py)


def test_flipL1_raises_as_the_reference_does():
    case = I.CASES["plain"]
    dev = torch.device("cuda:0")
    ts, host, E, R, gt = I.build(case, dev)
    ts.opt.flipL1 = True
    vinit = host.vertices_init.to(dev)
    with pytest.raises(RuntimeError, match="size of tensor"):
        ts.iteration(I.attributes_of({k: v.to(dev) for k, v in E.items()}, vinit),
                     lambda x: I.attributes_of({k: v.to(dev) for k, v in R.items()}, vinit))
