#!/usr/bin/env python3
"""Mints tests/golden/disentangle.npz: the reference's disentangle regularisation (the statements of /root/reference/trainer.py:455-494,
``lossR_dis = 0.0`` to ``lossR_dis += opt.dis2 * (l_cam + l_shape)``, which live inline in the training loop) EXECUTED here on seeded
attribute sets, with autograd's gradients.  The statements, ``fliplr`` and ``angle2xy`` (smr_utils.py) are read from the reference at
minting time and run with the loop's variables supplied by this script: ``netE`` hands out prepared attribute sets (first call: Ae_fliplr,
second: Ae_jitter), ``.cuda()`` is neutralised, ``torchvision.transforms.RandomErasing`` is a stub that returns its input.

So the golden pins the loss block and ``fliplr``.  It does NOT pin the erasing: ``draw_erase_box`` is restated from memory and held only
to its own call sequence (tests/test_disentangle_host.py).  Only inputs, the terms, ``lossR_dis`` and the gradients are committed.
Run from the repo root:  python tests/golden/make_golden_disentangle.py"""
import math
import os
import re
import textwrap
import types

import numpy as np
import torch

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BASE = ("textures", "vertices", "azimuths", "elevations", "distances", "biases", "delta_vertices")
FLIP = ("textures", "vertices")
JITTER = ("azimuths", "elevations", "distances", "biases", "delta_vertices")
CASES = ((0.7, 0.3, 2.0), (1.0, 0.0, 1.0), (0.0, 1.0, 1.0))          # (dis1, dis2, azim)
SHAPES = ((6, 5), (4, 8))                                            # (Ht, Wt)
B, V = 3, 5


def reference_block():
    lines = open(os.path.join(REF, "trainer.py")).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.strip() == "lossR_dis = 0.0")
    end = next(i for i, l in enumerate(lines) if "lossR_dis += opt.dis2 * (l_cam + l_shape)" in l)
    assert 0 < end - start < 60
    return textwrap.dedent("\n".join(lines[start:end + 1]))


def reference_function(name):
    src = open(os.path.join(REF, "smr_utils.py")).read()
    m = re.search(r"^def %s\(.*?(?=^\S)" % name, src, flags=re.M | re.S)
    return m.group(0)


def make_sets(Ht, Wt, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    def one():
        return {"textures": r(B, 3, Ht, Wt), "vertices": r(B, V, 3) - 0.5, "azimuths": r(B) * 360 - 180, "elevations": r(B) * 30,
                "distances": r(B) * 5 + 2, "biases": r(B, 2) * 0.6 - 0.3, "delta_vertices": (r(B, V, 3) - 0.5) * 0.2}
    Ae, Af, Aj = one(), one(), one()
    Af["vertices"][1] = Ae["vertices"][1] * torch.tensor([-1.0, 1.0, 1.0])         # one sample's flip difference is exactly zero
    Af["textures"][0, 1, 2] = Ae["textures"][0, 1, 2].flip(0)                     # ... and one texture row's texel differences
    return Ae, {k: Af[k] for k in FLIP}, {k: Aj[k] for k in JITTER}


def run_reference(code, helpers, Ae, Af, Aj, dis1, dis2, azim):
    leaf = lambda A: {k: v.clone().requires_grad_(True) for k, v in A.items()}
    Ae, Af, Aj = leaf(Ae), leaf(Af), leaf(Aj)
    answers = ([Af] if dis1 > 0 else []) + ([Aj] if dis2 > 0 else [])
    asked = []

    def netE(x, need_feats=False, img_pth=None):
        asked.append(tuple(x.shape))
        return answers[len(asked) - 1]

    tv = types.SimpleNamespace(transforms=types.SimpleNamespace(RandomErasing=lambda p=1: (lambda x: x)))
    env = dict(torch=torch, math=math, opt=types.SimpleNamespace(dis1=dis1, dis2=dis2, azim=azim, fp16=False, chamfer=False), Ae=Ae, netE=netE,
               Xa=torch.zeros(B, 4, 8, 8), img_path=None, torchvision=tv)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self          # the block's .cuda() calls, on a box without a GPU
    try:
        for h in helpers:
            exec(h, env)
        exec(code, env)
        env["lossR_dis"].backward()
    finally:
        torch.Tensor.cuda = cuda
    assert len(asked) == len(answers)
    grads = {}
    for name, A in (("Ae", Ae), ("Af", Af), ("Aj", Aj)):
        for k, v in A.items():
            if v.grad is not None:
                grads["grad_%s_%s" % (name, k)] = v.grad.numpy()
    return env, grads


def main():
    code = reference_block()
    helpers = [reference_function("fliplr"), reference_function("angle2xy")]
    out = {"cases": np.asarray(CASES, dtype=np.float64), "shapes": np.asarray(SHAPES, dtype=np.int64)}
    for si, (Ht, Wt) in enumerate(SHAPES):
        tag = "t%dx%d" % (Ht, Wt)
        Ae, Af, Aj = make_sets(Ht, Wt, seed=11 + si)
        for name, A in (("Ae", Ae), ("Af", Af), ("Aj", Aj)):
            for k, v in A.items():
                out["%s_%s_%s" % (tag, name, k)] = v.numpy()
        terms = np.zeros(7, np.float64)
        for ci, (dis1, dis2, azim) in enumerate(CASES):
            env, grads = run_reference(code, helpers, Ae, Af, Aj, dis1, dis2, azim)
            out["%s_c%d_lossR_dis" % (tag, ci)] = np.asarray(float(env["lossR_dis"].detach()), np.float64)
            for k, v in grads.items():
                out["%s_c%d_%s" % (tag, ci, k)] = v
            if dis2 == 0:                                    # l_shape is the flip half's here
                terms[0], terms[1] = float(env["l_text"].detach()), float(env["l_shape"].detach())
            if dis1 == 0:
                terms[2:] = [float(env[k].detach()) for k in ("loss_azim", "loss_elev", "loss_dist", "loss_bias", "l_shape")]
            if dis1 > 0 and dis2 > 0:
                assert sorted(k for k in grads if k.startswith("grad_Ae_")) == sorted("grad_Ae_" + k for k in BASE)   # all seven of Ae
        out[tag + "_terms"] = terms
        print(tag, terms)
    path = os.path.join(ROOT, "tests", "golden", "disentangle.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
