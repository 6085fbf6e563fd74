#!/usr/bin/env python3
"""Mints tests/golden/poisson_edit.npz: outputs of the reference's poisson_edit (/root/reference/poisson_image_editing.py) EXECUTED here
on small seeded uint8 images with offset (0, 0), for interior, border-touching, all-zero and all-one masks.  The reference's file is
loaded at minting time with a stub ``cv2`` whose ``warpAffine`` is the identity (all it is for a zero offset); only inputs and outputs
are committed.  Run from the repo root:  python tests/golden/make_golden_poisson.py"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference/poisson_image_editing.py"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = ((3, 3), (9, 7), (16, 12), (24, 16))
MASKS = ("interior", "border", "zero", "one")


def reference_module():
    cv2 = types.ModuleType("cv2")

    def warp_affine(src, M, size):
        assert not M[:, 2].any() and (M[:, :2] == np.eye(2)).all() and tuple(size) == (src.shape[1], src.shape[0])
        return src.copy()

    cv2.warpAffine = warp_affine
    sys.modules["cv2"] = cv2
    try:
        spec = importlib.util.spec_from_file_location("poisson_image_editing_reference", REF)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        del sys.modules["cv2"]
    return mod


def make_mask(kind, H, W, rng):
    m = np.zeros((H, W), dtype=np.uint8)
    if kind == "interior":                                   # an ellipse that stays off the outer rows and columns (3 x 3: the centre)
        yy, xx = np.mgrid[:H, :W]
        m[((yy - (H - 1) / 2) / max((H - 2) / 2 - 0.4, 0.5)) ** 2 + ((xx - (W - 1) / 2) / max((W - 2) / 2 - 0.4, 0.5)) ** 2 <= 1.0] = 255
        m[0], m[-1], m[:, 0], m[:, -1] = 0, 0, 0, 0
    elif kind == "border":                                   # touches all four edges and two corners, with holes; values other than 255 too
        m[: H // 2 + 1, W // 3:] = 200
        m[H // 3:, : W // 2 + 1] = 7
        m[rng.random((H, W)) < 0.15] = 0
        m[0, W - 1], m[H - 1, 0], m[0, W // 2], m[H // 2, 0], m[H - 1, W // 3], m[H // 3, W - 1] = 1, 1, 1, 1, 1, 1
    elif kind == "one":
        m[:] = 1
    return m


def main():
    ref = reference_module()
    rng = np.random.default_rng(20)
    out = {}
    for H, W in SHAPES:
        for kind in MASKS:
            key = "%dx%d_%s" % (H, W, kind)
            src = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            tgt = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            mask = make_mask(kind, H, W, rng)
            got = ref.poisson_edit(src.copy(), tgt.copy(), mask.copy(), (0, 0))      # (it writes into its target and its mask)
            assert got.dtype == np.uint8 and got.shape == (H, W, 3)
            out["source_" + key], out["target_" + key], out["mask_" + key], out["result_" + key] = src, tgt, mask, got
            print(key, "inside %d of %d" % (int((mask != 0).sum()), H * W), "bytes at 0 / 255:", int((got == 0).sum()), int((got == 255).sum()))
    path = os.path.join(ROOT, "tests", "golden", "poisson_edit.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
