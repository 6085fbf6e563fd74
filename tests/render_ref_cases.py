"""The edge cases shared by tests/test_render_ref_host.py (oracle against render_ref, float64) and tests/test_gpu_render_ref.py (device against
render_ref): seeded inputs on the repository's own layout (conftest.make_inputs), each bent towards the branch it is named for.  B = 2, at
most 40 pixels a side: render_ref is dense over (face, pixel) in its decisions.  Every value is an fp32 number, so the float64 reference,
the fp32 oracle and the device read the same inputs."""
import functools
import types

import numpy as np
import torch

import render_ref as R
from conftest import make_inputs

LEAVES = R.LEAVES
IMAGE_WEIGHT = 0.1                     # DiffRender's default
BASE_DISTANCES = (2.6, 3.4)            # close enough that faces span several pixels (test_oracle_gradcheck.py)


def _spec(template="sphere", S=32, ratio=1, no_mask=True, seed=0, device=True, **kw):
    return types.SimpleNamespace(template=template, S=S, ratio=ratio, no_mask=no_mask, seed=seed, device=device, kw=dict(R.DEFAULTS, **kw))


# name -> spec; `device`: the case is also run on the GPU (the regular ones: the template's own face table)
SPECS = {
    "sphere_bg": _spec(),
    "sphere_white": _spec(no_mask=False, seed=1),
    "uv_seams": _spec(template="smpl_uv_642", S=24, seed=2),
    "ratio2": _spec(template="smpl_uv_642", S=20, ratio=2, seed=3),                 # 40 x 20
    "cut_lists": _spec(seed=4, knum=3, boxlen=0.08, sigmainv=900.0),
    "deep_lists": _spec(seed=5, knum=30, boxlen=0.3),
    "uv_border": _spec(seed=6),
    "lights_x3": _spec(seed=7),
    "lights_neg": _spec(seed=8),
    "steep_elevation": _spec(seed=9),
    "close_camera": _spec(seed=10),
    "texture_1x3": _spec(seed=11),
    "texture_3x1": _spec(seed=12),
    "inside_out": _spec(seed=13, device=False),
    "coincident": _spec(seed=14, boxlen=0.08),                                      # (a point's box inflated by 0.02 * mult holds no 32-pixel centre)
    "depth_tie": _spec(seed=15, device=False),
}
DEVICE_CASES = tuple(k for k, s in SPECS.items() if s.device)


def _probe(inp, sp, H, W, proj):
    with torch.no_grad():
        return R.render_ref(inp, H, W, sp.no_mask, proj, **sp.kw)


def _border_pixels(fidx):
    """Uncovered pixels of image 0 with a covered 4-neighbour, in raster order: [(py, px)]."""
    cov = fidx[0] >= 0
    near = np.zeros_like(cov)
    near[1:] |= cov[:-1]; near[:-1] |= cov[1:]; near[:, 1:] |= cov[:, :-1]; near[:, :-1] |= cov[:, 1:]
    return np.argwhere(near & ~cov)


def _nearest_face(inp, sp, H, W, proj, py, px, skip=()):
    """The face of image 0 whose projected centroid is nearest to pixel (py, px)'s centre."""
    mult = sp.kw["mult"]
    T = R.camera(*(torch.as_tensor(inp[k], dtype=torch.float64) for k in ("azimuths", "elevations", "distances", "biases")))
    v = torch.as_tensor(inp["vertices"], dtype=torch.float64)
    vc = v @ T[:, :3] + T[:, 3:4]
    pr = torch.as_tensor(proj, dtype=torch.float64)
    vi = (vc[..., :2] * pr[:2] / (vc[..., 2:3] * pr[2]))[0] * mult
    cen = vi[torch.as_tensor(inp["faces"]).long()].mean(1)
    x0, y0 = mult / W * (2 * px + 1 - W), mult / H * (H - 2 * py - 1)
    d = (cen[:, 0] - x0) ** 2 + (cen[:, 1] - y0) ** 2
    for f in skip:
        d[f] = np.inf
    return int(d.argmin())


@functools.lru_cache(maxsize=None)
def build(name):
    """namespace: inp (numpy: fp32 arrays, int32 faces, face_uvs (F,3,2)), gt (B,4,H,W), proj (3,), H, W, no_mask, kw, spec, and
    collapsed (the coincident case: bool (F,), the faces of zero area; None elsewhere), twins (the groups of vertices moved onto one another)."""
    sp = SPECS[name]
    H, W = round(sp.ratio * sp.S), sp.S
    inp, gt, proj = make_inputs(sp.template, 2, H, W, seed=sp.seed, ratio=sp.ratio)
    inp = {k: v for k, v in inp.items() if k in LEAVES + ("faces", "face_uvs")}
    inp["face_uvs"] = np.ascontiguousarray(inp["face_uvs"].reshape(-1, 3, 2), dtype=np.float32)
    inp["distances"] = np.asarray(BASE_DISTANCES, np.float32)
    rng = np.random.default_rng(1000 + sp.seed)
    collapsed, twins = None, ()
    if name == "uv_border":
        inp["face_uvs"] = (inp["face_uvs"] * np.float32(1.6) - np.float32(0.3)).astype(np.float32)       # [-0.3, 1.3]: clamped on all four sides
    elif name == "lights_x3":
        inp["lights"] = inp["lights"] * np.float32(3)
    elif name == "lights_neg":
        # image 1 alone: with every light negated every pixel of an image saturates at 0 and its texture, light and background gradients are
        # exactly zero -- compared as such in image 1, while image 0 keeps each gradient's maximum non-zero
        inp["lights"] = inp["lights"] * np.asarray([[1.0], [-1.0]], np.float32)
    elif name == "steep_elevation":
        inp["elevations"] = np.asarray([89.0, -89.5], np.float32)
    elif name == "close_camera":
        inp["distances"] = np.asarray([1.2, 1.05], np.float32)
        # the mesh fills the screen but for its corners, which the target's ellipse does not reach: under the loss the background's whole gradient
        # would be the covered pixels' (1 - m) = eps / (sum + eps) = 1e-11, a rounding residue.  A target mask of ones gives the corners their gradient.
        gt = gt.copy()
        gt[:, 3] = 1
    elif name == "texture_1x3":
        inp["textures"] = rng.random((2, 3, 1, 3)).astype(np.float32)
    elif name == "texture_3x1":
        inp["textures"] = rng.random((2, 3, 3, 1)).astype(np.float32)
    elif name == "inside_out":
        inp["faces"] = np.ascontiguousarray(inp["faces"][:, ::-1])
        inp["face_uvs"] = np.ascontiguousarray(inp["face_uvs"][:, ::-1])
    elif name == "coincident":
        # one face collapsed to a point and, elsewhere, one edge collapsed -- by moving vertices onto one another, exactly, in both images; both
        # at image 0's silhouette, so that the soft mask's lists hold the collapsed faces (zero-length edges: t = 0)
        border = _border_pixels(_probe(inp, sp, H, W, proj)[1].numpy())
        v = inp["vertices"].copy()
        fa = _nearest_face(inp, sp, H, W, proj, *border[0])
        a, b, c = inp["faces"][fa]
        v[:, b] = v[:, a]; v[:, c] = v[:, a]
        touched = [f for f in range(inp["faces"].shape[0]) if set(inp["faces"][f]) & {a, b, c}]
        fb = _nearest_face(inp, sp, H, W, proj, *border[-1], skip=touched)
        d, e, _ = inp["faces"][fb]
        v[:, e] = v[:, d]
        inp["vertices"] = v
        twins = ((int(a), int(b), int(c)), (int(d), int(e)))
        tri = v[0][inp["faces"]].astype(np.float64)
        collapsed = (np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) == 0).all(1)
    elif name == "depth_tie":
        # two coplanar copies of one face, twice: the copy above its original in the table (the original wins) and below it (the copy wins);
        # the copies keep their own texture coordinates, so the wrong winner shows in the image
        fidx = _probe(inp, sp, H, W, proj)[1].numpy()
        faces = inp["faces"].copy()
        i = int(fidx[0, H // 2, W // 2]); j = int(fidx[0, H // 2 - 3, W // 2 + 3])
        assert i >= 0 and j >= 5 and abs(i - j) > 8
        faces[i + 5] = faces[i]
        faces[j - 5] = faces[j]
        inp["faces"] = faces
    return types.SimpleNamespace(name=name, inp=inp, gt=gt, proj=np.asarray(proj, np.float32).reshape(3), H=H, W=W, no_mask=sp.no_mask, kw=sp.kw,
                                 spec=sp, collapsed=collapsed, twins=twins)


def upstream_noise(case, zero_collapsed=True):
    """Seeded N(0,1) on rgba (B,H,W,4) and on the face normals (B,F,3), fp32 numbers; zero on the collapsed faces' normals unless asked."""
    rng = np.random.default_rng(77 + case.spec.seed)
    w = rng.normal(size=(2, case.H, case.W, 4)).astype(np.float32)
    wfn = rng.normal(size=(2, case.inp["faces"].shape[0], 3)).astype(np.float32)
    if case.collapsed is not None and zero_collapsed:
        wfn[:, case.collapsed] = 0
    return w, wfn


def as64(inp):
    return {k: (None if v is None else (v.astype(np.float64) if v.dtype == np.float32 else v)) for k, v in inp.items()}


def leaves(case):
    return [k for k in LEAVES if not (k == "bg" and not case.no_mask)]


def merge_twins(case, g):
    """A vertex gradient with every group of coincident vertices given the group's SUM.  A face collapsed to a segment has two edges that are
    one segment walked both ways: the pixel's distances to them are equal in exact arithmetic, the closer one is chosen by the last bit, and
    with it WHICH of two coincident corners takes the soft mask's gradient.  What is defined is the gradient of the shared position."""
    g = np.array(g, dtype=np.float64)
    for grp in case.twins:
        g[:, list(grp)] = g[:, list(grp)].sum(1, keepdims=True)
    return g


CONTOUR = {"loss": 0.0, "loss_contour": 0.3}


def _oracle():
    import oracle
    oracle.lib()
    return oracle


def upstream_of(case, up, rgba, dtype):
    """(drgba (B,H,W,4), dface_normals or None) at `dtype`: noise, or recon_data's own gradient on `rgba` (B,H,W,4) at that dtype."""
    if up in ("noise", "noise_all"):
        w, wfn = upstream_noise(case, zero_collapsed=(up == "noise"))
        return w.astype(dtype), wfn.astype(dtype)
    _, dpred = _oracle().recon_data(rgba.transpose(0, 3, 1, 2), case.gt.astype(dtype), image_weight=IMAGE_WEIGHT, contour=CONTOUR[up],
                                    want_grad=True, dtype=dtype)
    return np.ascontiguousarray(dpred.transpose(0, 2, 3, 1)), None


def reference(case, w, wfn, face_idx=None, faults=()):
    """render_ref on the case's inputs and its gradients under (w, wfn): namespace rgba, fidx, fn, imn (arrays), grads {leaf: array}, cnt."""
    L = R.leaves_of(case.inp, case.no_mask)
    rgba, fidx, fn, imn, cnt = R.render_ref(L, case.H, case.W, case.no_mask, case.proj, face_idx=face_idx, faults=faults, **case.kw)
    y = (rgba * torch.from_numpy(np.asarray(w, np.float64))).sum()
    if wfn is not None:
        y = y + (fn * torch.from_numpy(np.asarray(wfn, np.float64))).sum()
    y.backward()
    return types.SimpleNamespace(rgba=rgba.detach().numpy(), fidx=fidx.numpy(), fn=fn.detach().numpy(), imn=imn.detach().numpy(),
                                 grads={k: (np.zeros(tuple(L[k].shape)) if L[k].grad is None else L[k].grad.numpy()) for k in leaves(case)}, cnt=cnt)


def oracle_run(case, up, dtype):
    o = _oracle()
    inp = as64(case.inp) if dtype == np.float64 else case.inp
    proj = case.proj.astype(dtype)
    rgba, fidx, fn, imn = o.render_forward(inp, case.H, case.W, case.no_mask, proj, dtype=dtype, **case.kw)
    w, wfn = upstream_of(case, up, rgba, dtype)
    g = o.render_backward(inp, case.H, case.W, case.no_mask, proj, w, wfn, dtype=dtype, **case.kw)
    return types.SimpleNamespace(rgba=rgba, fidx=fidx, fn=fn, imn=imn, grads=g, w=w, wfn=wfn)
