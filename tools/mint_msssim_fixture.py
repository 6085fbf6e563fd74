#!/usr/bin/env python3
"""Mint the fixture that PINS ssim.py to the real pytorch_msssim.  Runs only where pytorch_msssim is installed (any device torch has:
the numbers are computed in fp64 on the host, so no GPU is needed).  A maintainer with such a machine runs

    python tools/mint_msssim_fixture.py            # writes tests/golden/msssim_fixture.npz (~1.5 MB)

and commits the file; tests/test_gpu_ssim.py::test_matches_real_pytorch_msssim_fixture then stops skipping and checks the MI355X op
against it: per-image values within 1e-5, gradients to X and Y within parity_bar.grad_close.

What is recorded, per case: seeded fp32 inputs X and Y, data_range, pytorch_msssim's per-image value (size_average=False) and the
gradients of its sum with respect to X and Y.  Nothing of pytorch_msssim's source is stored -- numbers only.
"""
import argparse
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (shape, data_range); names starting with "ms" go through ms_ssim
CASES = {"ssim_eval": ((1, 3, 128, 128), 1.0), "ssim_batch": ((4, 3, 64, 96), 1.0), "ssim_skip": ((2, 1, 7, 60), 1.0),
         "ssim_255": ((2, 3, 48, 48), 255.0), "ms_176": ((2, 3, 176, 176), 1.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "msssim_fixture.npz"))
    args = ap.parse_args()
    import pytorch_msssim                                          # the real package: there is nothing to pin against without it
    out = {}
    for i, (name, (shape, dr)) in enumerate(CASES.items()):
        g = torch.Generator().manual_seed(1000 + i)
        X = torch.rand(shape, generator=g)
        Y = (0.7 * X + 0.3 * torch.rand(shape, generator=g) + 0.15 * torch.randn(shape, generator=g)).clamp(0, 1)
        X, Y = (X * dr).float(), (Y * dr).float()
        fn = pytorch_msssim.ms_ssim if name.startswith("ms") else pytorch_msssim.ssim
        X64, Y64 = X.double().requires_grad_(True), Y.double().requires_grad_(True)
        v = fn(X64, Y64, data_range=dr, size_average=False)
        v.sum().backward()
        out.update({name + "_X": X.numpy(), name + "_Y": Y.numpy(), name + "_data_range": np.float64(dr),
                    name + "_val": v.detach().numpy(), name + "_gX": X64.grad.numpy(), name + "_gY": Y64.grad.numpy()})
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, "pytorch_msssim", getattr(pytorch_msssim, "__version__", "?"))


if __name__ == "__main__":
    main()
