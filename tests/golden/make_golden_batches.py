"""Mints tests/golden/input_batches.npz: the outputs of the reference's own loaders on seeded images.

    python tests/golden/make_golden_batches.py <root of the reference checkout>

Needs the reference's ``datasets/bird.py`` and ``datasets/market.py``, Pillow and torch; it is run where those exist, and only the
data it writes is committed.  ``CUBDataset.__getitem__`` and ``MarketDataset.__getitem__`` are run as they are on instances made with
``object.__new__`` whose attributes are set by hand; their two loaders return Pillow images built from seeded arrays; ``torchvision``
and ``kaolin`` are ``sys.modules`` stubs (``to_tensor`` is the only function the loaders call); the datasets' ``random`` is a proxy
that forwards to a seeded ``random.Random`` and writes down what was drawn.

Per case k the file holds: c<k>_recipe, _train, _bg, _seed, _out_hw (H, W), _n, the sources _img<i> (H,W,3) and _seg<i> (H,W) uint8,
_draws -- (n,7) int32 rows (flip, w, h, left, upper, right, lower) for cub, (n,3) rows (left, upper, flip) for market, (n,0) when
nothing is drawn -- and _out (n,4,H,W) float32, the tensors the loader returned."""
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def to_tensor(pic):
    a = np.array(pic, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(torch.float32).div(255)


def stub_modules():
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.functional = types.ModuleType("torchvision.transforms.functional")
    tv.transforms.functional.to_tensor = to_tensor
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms, "torchvision.transforms.functional": tv.transforms.functional,
                        "kaolin": types.ModuleType("kaolin")})


def load(root, name):
    spec = importlib.util.spec_from_file_location("reference_" + name, os.path.join(root, "datasets", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Draws:
    """stands in for the ``random`` module inside a dataset module"""

    def __init__(self, seed):
        self.rng, self.log = random.Random(seed), []

    def uniform(self, a, b):
        v = self.rng.uniform(a, b)
        self.log.append(("uniform", v))
        return v

    def randint(self, a, b):
        v = self.rng.randint(a, b)
        self.log.append(("randint", v))
        return v


def sources(rng, shapes):
    imgs, segs = [], []
    for Hs, Ws in shapes:
        img = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
        u = rng.random((Hs, Ws, 3))
        img[u < 0.25], img[u > 0.75] = 0, 255
        # blobs, so that the mask is not pure noise, with the threshold's neighbours 160 and 161 among the values
        yy, xx = np.mgrid[:Hs, :Ws]
        inside = ((yy - Hs / 2.0) / (0.4 * Hs + 1)) ** 2 + ((xx - Ws / 2.0) / (0.4 * Ws + 1)) ** 2 < 1.0
        seg = np.where(inside, rng.choice(np.array([161, 255, 255, 255], dtype=np.uint8), (Hs, Ws)), rng.choice(np.array([0, 0, 0, 160], dtype=np.uint8), (Hs, Ws)))
        imgs.append(img)
        segs.append(seg.astype(np.uint8))
    return imgs, segs


CASES = (  # recipe, train, bg, image_size, source shapes (H, W)
    ("cub", True, False, 16, ((48, 64), (23, 37))),
    ("cub", True, True, 32, ((20, 13),)),
    ("cub", False, False, 32, ((17, 24),)),
    ("cub", False, True, 16, ((7, 5), (25, 25))),
    ("market", True, False, 16, ((48, 24), (31, 17))),
    ("market", True, True, 16, ((64, 32),)),
    ("market", False, False, 16, ((40, 21),)),
    ("market", False, True, 16, ((9, 6), (32, 16))),
)


def main(root):
    stub_modules()
    mods = {"cub": load(root, "bird"), "market": load(root, "market")}
    out = {"n_cases": np.int32(len(CASES))}
    for k, (recipe, train, bg, size, shapes) in enumerate(CASES):
        seed = 100 + k
        imgs, segs = sources(np.random.default_rng(seed), shapes)
        mod = mods[recipe]
        ds = object.__new__(mod.CUBDataset if recipe == "cub" else mod.MarketDataset)
        ds.selected_index, ds.image_size, ds.train, ds.aug, ds.bg, ds.hmr = [], size, train, train, bg, 0.0
        ds.imgs = [("%03d_0.50.png" % i, 0) for i in range(len(imgs))]
        ds.loader = lambda path: Image.fromarray(imgs[int(os.path.basename(path)[:3])], "RGB")
        ds.seg_loader = lambda path: Image.fromarray(segs[int(os.path.basename(path)[:3])], "L")
        draws = mod.random = Draws(seed)
        tensors, rows = [], []
        for i in range(len(imgs)):
            draws.log = []
            tensors.append(ds[i]["data"]["images"].numpy())
            kinds, vals = [d[0] for d in draws.log], [d[1] for d in draws.log]
            if not train:
                assert not vals
                rows.append([])
            elif recipe == "cub":
                assert kinds == ["uniform"] + ["randint"] * 6
                rows.append([int(vals[0] < 0.5)] + vals[1:])
            else:
                assert kinds == ["randint", "randint", "uniform"]
                rows.append(vals[:2] + [int(vals[2] < 0.5)])
        p = "c%02d_" % k
        H, W = (size, size) if recipe == "cub" else (2 * size, size)
        res = np.stack(tensors)
        assert res.shape == (len(imgs), 4, H, W) and res.dtype == np.float32
        out.update({p + "recipe": np.array(recipe), p + "train": np.bool_(train), p + "bg": np.bool_(bg), p + "seed": np.int64(seed),
                    p + "out_hw": np.array([H, W], dtype=np.int32), p + "n": np.int32(len(imgs)),
                    p + "draws": np.array(rows, dtype=np.int32).reshape(len(imgs), -1), p + "out": res})
        for i in range(len(imgs)):
            out[p + "img%d" % i], out[p + "seg%d" % i] = imgs[i], segs[i]
    path = os.path.join(HERE, "input_batches.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
