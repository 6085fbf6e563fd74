"""The backward's pixel pass must not depend on the order in which the GPU starts workgroups (advisor, round 3): a pixel lane that does not
find its texture tile's record-list offset -- normally published by the image's plan workgroup of the same launch -- forms it from the
forward's per-tile counts itself.  A TEST build of the library in which the plan workgroups publish their offsets ~0.3 ms late and the lanes give up after four polls
(build_native.TEST_LIB_SELF_OFFSETS, built by __graft_entry__.build()) takes that path for every record; its gradients must be the
product's bit for bit (the texture gather sums in integer fixed point, so not even the order of the records matters), no record may be
reported as dropped."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

_SCRIPT = r"""
import importlib, os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
pkg = importlib.import_module("3d-magic-mirror_amd")
if sys.argv[3] != "-":
    pkg._native.LIB_PATH = sys.argv[3]                # (the C++ nodes resolve every library function through _native.lib(): this build)
    assert pkg._native.lib()._name == sys.argv[3]
dev = torch.device("cuda:0")
out = {}
for name, B, S in (("sphere", 3, 64), ("smpl_uv_642", 4, 128)):
    dr = pkg.DiffRender(os.path.join(sys.argv[1], "tests", "golden", "templates", name + ".npz"), S, emit_imnormal=True)
    att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, B, S, S, seed=5)
    leaves = ("vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases")
    datt = {k: (v.to(dev).requires_grad_(k in leaves) if torch.is_tensor(v) else v) for k, v in att.items()}
    rgbs, _ = dr.render(no_mask=True, **datt)
    loss = dr.recon_data(rgbs, gt.to(dev), no_mask=True)
    loss.backward()
    torch.cuda.synchronize()
    out[name + "_dropped"] = np.int64(dr.poll_dropped_records())
    out[name + "_loss"] = loss.detach().cpu().numpy()
    for k in leaves:
        out[name + "_" + k] = datt[k].grad.cpu().numpy()
np.savez(sys.argv[2], **out)
"""


def _run(tmp_path, tag, libpath):
    dst = str(tmp_path / (tag + ".npz"))
    r = subprocess.run([sys.executable, "-c", _SCRIPT, ROOT, dst, libpath], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(dst)


@pytest.mark.timeout(900)
def test_the_backward_does_not_depend_on_the_plan_workgroups_running_first(tmp_path):
    bn = importlib.import_module("3d-magic-mirror_amd.build_native")
    lib = bn.TEST_LIB_SELF_OFFSETS
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(bn.LIB):
        lib = bn.build_test_variants()                           # needs hipcc: a box without it FAILS here rather than skipping
    product = _run(tmp_path, "product", "-")
    selfoff = _run(tmp_path, "selfoff", lib)
    assert set(product.files) == set(selfoff.files)
    for k in product.files:
        if k.endswith("_dropped"):
            assert int(product[k]) == 0 and int(selfoff[k]) == 0, k
        else:
            assert np.array_equal(product[k], selfoff[k]), k     # bit for bit
    assert float(np.abs(product["smpl_uv_642_textures"]).max()) > 0
