"""DiffRender.render restated in torch float64 with the DERIVATIVE left to autograd: the independent pin of the C oracle's hand-derived
render_backward (oracle/mm_oracle.inc) and, through `face_idx=`, a direct float64 yardstick for the device.  A plain
helper module (like parity_bar.py and iteration_ref.py) for tests/test_render_ref_host.py and tests/test_gpu_render_ref.py.  It needs torch
alone: it does not import the oracle, and it is written from SURVEY 8(a) a2-a10, not from the oracle's backward.

What is differentiable: the camera, [v,1] @ T, the projection, the gather by faces, the face normals n / (|n| + 1e-10), the barycentrics of
the covered pixels, the features [1, uv, normal], F.grid_sample(bilinear, border, align_corners=False), the nine SH bands, both composites,
the clamp, and the soft mask 1 - prod(1 - exp(-d2 / mult^2 * sigmainv)).  What is DECIDED, under torch.no_grad() and by brute force over
(face, pixel): validity (fn_z >= 0), the closed bounding boxes, coverage (all three weights >= 0), the depth test (largest interpolated z,
lowest face index on a tie), the soft mask's list (the first knum faces in index order whose box inflated by boxlen * mult holds the pixel,
culled faces included), and per list entry the closest edge and its region.  A decision has no derivative; everything else has autograd's.

Two places are written NaN-safe, with the `where` on both sides of the division, because autograd's plain form gives 0 * inf there: the
length of a zero face normal (the oracle's convention: the direction term is 0, the gradient is dn / 1e-10) and the projection parameter of
a zero-length edge (t = 0).

FAULTS names one deliberately wrong derivative at a time (forward values unchanged), each applied by detaching or rewriting the one term it
names; tests/test_render_ref_host.py shows that each of them is visible far above the bar of the GPU test."""
import math

import numpy as np
import torch
import torch.nn.functional as F_

LEAVES = ("vertices", "textures", "lights", "bg", "azimuths", "elevations", "distances", "biases")
FAULTS = ("soft_vertex_regions_dropped", "soft_excl_includes_self", "soft_skips_culled", "clamp_passes_gradient",
          "border_uv_gradient_not_gated", "normal_eps_dropped", "bary_eps_dropped", "elevation_chain_dropped", "bg_weight_wrong")
DEFAULTS = dict(sigmainv=7000.0, boxlen=0.02, knum=30, mult=1000.0, eps=1e-8)
SH = (0.28209479177, 0.4886025119, 1.09254843059, 0.94617469575, 0.31539156525, 0.77254840404, 0.38627420202)


def _t(a):
    if torch.is_tensor(a):
        return a if a.dtype == torch.float64 else a.to(torch.float64)
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def _straight_through(value, slope):
    """`value`'s number with `slope`'s derivative."""
    return slope + (value - slope).detach()


def leaves_of(inp, no_mask):
    """The inputs as float64 leaf tensors that require grad (bg only where a render reads it); faces and face_uvs as plain tensors."""
    out = {}
    for k in LEAVES:
        if k == "bg" and (not no_mask or inp.get(k) is None):
            out[k] = None
            continue
        a = inp[k]
        a = a.detach().cpu() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
        out[k] = a.to(torch.float64).clone().requires_grad_(True)
    f = inp["faces"]
    out["faces"] = (f.detach().cpu() if torch.is_tensor(f) else torch.from_numpy(np.asarray(f))).long()
    out["face_uvs"] = _t(inp["face_uvs"].detach().cpu() if torch.is_tensor(inp["face_uvs"]) else inp["face_uvs"]).reshape(-1, 3, 2)
    return out


def camera(azimuths, elevations, distances, biases, faults=()):
    """T (B,4,3): rows 0-2 the look-at rotation's columns x, y, z; row 3 = -cam @ R.  up = (0,1,0), at = (bias, 0)."""
    d2r = math.pi / 180.0
    elev = elevations.detach() if "elevation_chain_dropped" in faults else elevations
    er, ar = elev * d2r, azimuths * d2r
    ce, se, ca, sa = torch.cos(er), torch.sin(er), torch.cos(ar), torch.sin(ar)
    cam = torch.stack([distances * ce * sa, distances * se, distances * ce * ca], 1)
    at = torch.cat([biases, torch.zeros_like(biases[:, :1])], 1)
    up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).expand_as(cam)
    z = cam - at
    z = z / z.norm(dim=1, keepdim=True)
    x = torch.cross(up, z, dim=1)
    x = x / x.norm(dim=1, keepdim=True)
    y = torch.cross(z, x, dim=1)
    R = torch.stack([x, y, z], 2)
    return torch.cat([R, -(cam[:, None, :] @ R)], 1)


def _bary(s, x0, y0, eps, faults=()):
    """s (...,3,2) in mult units, x0 / y0 (...): the three edge functions over their sum plus copysign(eps)."""
    ax, ay, bx, by, cx, cy = (s[..., 0, 0] - x0, s[..., 0, 1] - y0, s[..., 1, 0] - x0, s[..., 1, 1] - y0, s[..., 2, 0] - x0, s[..., 2, 1] - y0)
    k = torch.stack([bx * cy - by * cx, cx * ay - cy * ax, ax * by - ay * bx], -1)
    tot = (k[..., 0] + k[..., 1]) + k[..., 2]
    nrm = tot + torch.copysign(torch.full_like(tot, eps), tot.detach())
    w = k / nrm[..., None]
    if "bary_eps_dropped" in faults:
        ok = tot.detach() != 0
        plain = k / torch.where(ok, tot, torch.ones_like(tot))[..., None]
        w = torch.where(ok[..., None], _straight_through(w, plain), w)
    return w


def _seg(px, py, u, v):
    """Squared distance from (px, py) to the segment u -> v by clamped projection, and the region (0: first end, 1: interior, 2: second end)."""
    ex, ey, rx, ry = v[..., 0] - u[..., 0], v[..., 1] - u[..., 1], px - u[..., 0], py - u[..., 1]
    len2 = ex * ex + ey * ey
    ok = len2.detach() > 0
    t = torch.where(ok, (rx * ex + ry * ey) / torch.where(ok, len2, torch.ones_like(len2)), torch.zeros_like(len2))
    with torch.no_grad():
        reg = torch.where(t <= 0, 0, torch.where(t >= 1, 2, 1))
    # the ends' distances are |p - u|^2 and |p - v|^2 as such (not p - (u + 1 * e)): two edges that end in the same point tie EXACTLY, and the
    # caller's strict < then keeps the lowest edge -- the oracle's convention for which of two coincident corners takes the gradient
    qx = torch.where(reg == 1, px - (u[..., 0] + t * ex), torch.where(reg == 2, px - v[..., 0], rx))
    qy = torch.where(reg == 1, py - (u[..., 1] + t * ey), torch.where(reg == 2, py - v[..., 1], ry))
    return qx * qx + qy * qy, reg


def _pixels(H, W, mult):
    p = torch.arange(H * W)
    x0 = (mult / W) * (2 * (p % W) + 1 - W).to(torch.float64)
    y0 = (mult / H) * (H - 2 * torch.div(p, W, rounding_mode="floor") - 1).to(torch.float64)
    return x0, y0


def render_ref(inp, H, W, no_mask, proj, *, sigmainv, boxlen, knum, mult, eps, face_idx=None, faults=()):
    """inp: dict with vertices (B,V,3), faces (F,3), face_uvs (F,3,2), textures (B,3,Ht,Wt), lights (B,9), bg (B,3,H,W) or None, azimuths,
    elevations, distances (B,), biases (B,2): float64 tensors (leaves_of makes them) or arrays.  proj: the three projection factors.
    Returns rgba (B,H,W,4), face_idx (B,H,W) int32, face_normals (B,F,3), imnormal (B,H,W,3), counters (dict of ints)."""
    faults = tuple(faults)
    assert all(f in FAULTS for f in faults), faults
    v, tex, lights = _t(inp["vertices"]), _t(inp["textures"]), _t(inp["lights"])
    faces = torch.as_tensor(np.asarray(inp["faces"]) if not torch.is_tensor(inp["faces"]) else inp["faces"]).long()
    fuv = _t(inp["face_uvs"]).reshape(-1, 3, 2)
    bg = _t(inp["bg"]) if (no_mask and inp.get("bg") is not None) else None
    assert bg is not None or not no_mask
    proj = _t(proj).reshape(3)
    B, P = v.shape[0], H * W
    Ht, Wt = tex.shape[2:]

    # a2-a5: camera, projection, gather, face normals
    T = camera(_t(inp["azimuths"]), _t(inp["elevations"]), _t(inp["distances"]), _t(inp["biases"]), faults)
    vc = v @ T[:, :3] + T[:, 3:4]
    vi = vc[..., :2] * proj[:2] / (vc[..., 2:3] * proj[2])
    fvc, fvi = vc[:, faces], vi[:, faces]                               # (B,F,3,3), (B,F,3,2)
    n = torch.cross(fvc[:, :, 1] - fvc[:, :, 0], fvc[:, :, 2] - fvc[:, :, 0], dim=2)
    n2 = (n * n).sum(2, keepdim=True)
    flat = n2.detach() == 0                                             # a collapsed face: |n| is the constant 0, the gradient dn / 1e-10
    length = torch.where(flat, torch.zeros_like(n2), torch.sqrt(torch.where(flat, torch.ones_like(n2), n2)))
    fn = n / (length + 1e-10)
    if "normal_eps_dropped" in faults:
        fn = _straight_through(fn, n / torch.where(flat, torch.ones_like(n2), length))
    s = fvi * mult
    x0, y0 = _pixels(H, W, mult)

    # a8: the decisions
    cnt = dict(cut_pixels=0, zero_length_edges=0, region_first=0, region_interior=0, region_second=0, culled_entries=0, list_entries=0, depth_ties=0,
               u_clamped_lo=0, u_clamped_hi=0, v_clamped_lo=0, v_clamped_hi=0, rgb_clamped_0=0, rgb_clamped_1=0, covered=0)
    fmap = torch.empty(B, P, dtype=torch.long)
    entries = []
    with torch.no_grad():
        valid = fn[..., 2] >= 0
        for b in range(B):
            sb = s[b]
            sx, sy = sb[..., 0], sb[..., 1]
            xmin, xmax, ymin, ymax = sx.min(1)[0][:, None], sx.max(1)[0][:, None], sy.min(1)[0][:, None], sy.max(1)[0][:, None]
            if face_idx is None:
                w = _bary(sb[:, None], x0[None], y0[None], eps)                                            # (F,P,3)
                inside = (x0 >= xmin) & (x0 <= xmax) & (y0 >= ymin) & (y0 <= ymax) & (w >= 0).all(-1) & valid[b][:, None]
                zb = fvc[b, :, :, 2]
                depth = (w[..., 0] * zb[:, 0:1] + w[..., 1] * zb[:, 1:2]) + w[..., 2] * zb[:, 2:3]
                depth = torch.where(inside, depth, torch.full_like(depth, -math.inf))
                best = depth.max(0)[0]
                hit = best > -math.inf
                fmap[b] = torch.where(hit, torch.argmax(depth, 0), torch.full((P,), -1, dtype=torch.long))   # argmax: the FIRST maximal index
                cnt["depth_ties"] += int((((depth == best) & hit).sum(0) > 1).sum())
                del w, inside, depth
            else:
                fmap[b] = torch.as_tensor(np.array(face_idx[b].cpu() if torch.is_tensor(face_idx) else face_idx[b])).long().reshape(P)
            infl = boxlen * mult
            cand = (x0 >= xmin - infl) & (x0 <= xmax + infl) & (y0 >= ymin - infl) & (y0 <= ymax + infl) & (fmap[b] < 0)
            rank = cand.cumsum(0)
            cnt["cut_pixels"] += int((rank[-1] > knum).sum())
            e = (cand & (rank <= knum)).t().nonzero()                                                       # [pixel, face], pixel-major
            entries.append(torch.cat([torch.full((e.shape[0], 1), b, dtype=torch.long), e], 1))
            del cand, rank
    entries = torch.cat(entries, 0)
    eb, ep, ef = entries[:, 0], entries[:, 1], entries[:, 2]
    cov = fmap >= 0
    cnt["covered"] = int(cov.sum())

    # a8: the covered pixels' barycentrics and features [1, uv, normal]
    fsel = fmap.clamp(min=0)
    bsel = torch.arange(B)[:, None].expand(B, P)
    w = _bary(s[bsel, fsel], x0[None].expand(B, P), y0[None].expand(B, P), eps, faults)
    w = torch.where(cov[..., None], w, torch.zeros_like(w))                                                 # (B,P,3)
    m = (w[..., 0] + w[..., 1]) + w[..., 2]
    uv = (w[..., None] * fuv[fsel]).sum(2)                                                                  # (B,P,2)
    imn = (w[..., None] * fn[bsel, fsel][:, :, None, :]).sum(2)                                             # (B,P,3)

    # a9: texture_mapping = grid_sample on (2u - 1, -(2v - 1))
    grid = torch.stack([uv[..., 0] * 2 - 1, -(uv[..., 1] * 2 - 1)], -1)
    with torch.no_grad():
        ix, iy = ((grid[..., 0] + 1) * Wt - 1) / 2, ((grid[..., 1] + 1) * Ht - 1) / 2
        cnt["u_clamped_lo"], cnt["u_clamped_hi"] = int(((ix <= 0) & cov).sum()), int(((ix >= Wt - 1) & cov).sum())
        cnt["v_clamped_hi"], cnt["v_clamped_lo"] = int(((iy <= 0) & cov).sum()), int(((iy >= Ht - 1) & cov).sum())    # v runs against iy
    if "border_uv_gradient_not_gated" in faults:
        tc = _bilinear_ungated(tex, grid)
    else:
        tc = F_.grid_sample(tex, grid[:, None], mode="bilinear", padding_mode="border", align_corners=False)[:, :, 0].permute(0, 2, 1)

    # a10: nine SH bands, the oracle's default order (x, z, y in the linear band)
    x, y, z = imn[..., 0], imn[..., 1], imn[..., 2]
    c0, c1, c4, c6, c6b, c7, c8 = SH
    bands = torch.stack([torch.full_like(x, c0), c1 * x, c1 * z, c1 * y, c4 * (x * y), c4 * (y * z), c6 * (z * z) - c6b, c7 * (x * z),
                         c8 * (x * x - y * y)], -1)
    cf = (bands * lights[:, None, :]).sum(-1)                                                               # (B,P)

    # the composites and the clamp
    mm, cc = m[..., None], cf[..., None]
    if no_mask:
        bgp = bg.reshape(B, 3, P).permute(0, 2, 1)
        if "bg_weight_wrong" in faults:
            back = _straight_through((bgp * (1 - mm)) * cc, bgp + (bgp.detach() * (1 - mm)) * cc)        # d/dbg = 1
            pre = (tc * mm) * cc + back
        else:
            pre = (tc * mm + bgp * (1 - mm)) * cc
    else:
        pre = (tc * mm) * cc + (1 - mm)
    rgb = pre.clamp(0, 1)
    if "clamp_passes_gradient" in faults:
        rgb = _straight_through(rgb, pre)
    cnt["rgb_clamped_0"], cnt["rgb_clamped_1"] = int((pre.detach() < 0).sum()), int((pre.detach() > 1).sum())

    # a8: the soft mask over the kept list entries
    alpha = cov.to(torch.float64)
    if entries.shape[0]:
        se, ex0, ey0 = s[eb, ef], x0[ep], y0[ep]
        d2, reg = None, None
        cnt["zero_length_edges"] = int(((se - se.roll(-1, 1)).detach().abs().sum(-1) == 0).sum())
        for k in range(3):
            dk, rk = _seg(ex0, ey0, se[:, k], se[:, (k + 1) % 3])
            if d2 is None:
                d2, reg = dk, rk
            else:
                closer = dk.detach() < d2.detach()                      # strict: the lowest edge on a tie
                d2, reg = torch.where(closer, dk, d2), torch.where(closer, rk, reg)
        if "soft_vertex_regions_dropped" in faults:
            d2 = torch.where(reg == 1, d2, d2.detach())
        prob = torch.exp(-(d2 / (mult * mult)) * sigmainv)
        culled = ~valid[eb, ef]
        if "soft_skips_culled" in faults:
            prob = torch.where(culled, prob.detach(), prob)
        for r, name in enumerate(("region_first", "region_interior", "region_second")):
            cnt[name] = int((reg == r).sum())
        cnt["culled_entries"], cnt["list_entries"] = int(culled.sum()), int(entries.shape[0])
        # (pixel, slot) table, unused slots p = 0
        pix = eb * P + ep
        first = torch.ones_like(pix, dtype=torch.bool)
        first[1:] = pix[1:] != pix[:-1]
        start = torch.nonzero(first)[:, 0]
        row = torch.cumsum(first.long(), 0) - 1
        slot = torch.arange(pix.shape[0]) - start[row]
        table = torch.zeros(start.shape[0], knum, dtype=torch.float64).index_put((row, slot), prob)
        keep = (1 - table).prod(1)
        soft = 1 - keep
        if "soft_excl_includes_self" in faults:
            soft = _straight_through(soft, (keep.detach()[:, None] * table).sum(1))
        alpha = alpha.reshape(-1).index_put((pix[start],), soft).reshape(B, P)
    rgba = torch.cat([rgb, alpha[..., None]], -1).reshape(B, H, W, 4)
    return rgba, fmap.reshape(B, H, W).to(torch.int32), fn, imn.reshape(B, H, W, 3), cnt


def _bilinear_ungated(tex, grid):
    """grid_sample(bilinear, border, align_corners=False)'s values with the border clamp's gradient gate left out (the fault): (B,P,3)."""
    B, C, Ht, Wt = tex.shape
    ix, iy = ((grid[..., 0] + 1) * Wt - 1) / 2, ((grid[..., 1] + 1) * Ht - 1) / 2
    ix = _straight_through(ix.clamp(0, Wt - 1), ix)
    iy = _straight_through(iy.clamp(0, Ht - 1), iy)
    fx, fy = ix.detach().floor(), iy.detach().floor()
    tx, ty = ix - fx, iy - fy
    x0, y0 = fx.long(), fy.long()
    b = torch.arange(B)[:, None]
    t = tex.permute(0, 2, 3, 1)

    def at(yy, xx):
        ok = ((xx < Wt) & (yy < Ht))[..., None]
        return torch.where(ok, t[b, yy.clamp(max=Ht - 1), xx.clamp(max=Wt - 1)], torch.zeros((), dtype=tex.dtype))
    ex, ey = (1 - tx)[..., None], (1 - ty)[..., None]
    tx, ty = tx[..., None], ty[..., None]
    return at(y0, x0) * ex * ey + at(y0, x0 + 1) * tx * ey + at(y0 + 1, x0) * ex * ty + at(y0 + 1, x0 + 1) * tx * ty
