// mm_pixel_pass.h -- the arithmetic of the backward's pixel-major pass, ONE text for its two homes:
//   pixel_bwd_kernel (mm_pixel_bwd.hip)        re-loads and re-forms the forward's per-pixel quantities, then calls these
//   shade_store / shade_empty_tiles in STEP MODE (mm_raster_common.h, MMRenderDesc.step_grads)   calls them on the values the epilogue holds
// Both translation units are compiled with the forward's floating-point flags (no contraction, IEEE division): the same expressions in the same
// order give the same bits in both, which is what lets a step-mode build be compared bit for bit with the standalone pass.
#pragma once
#include "mm_device.h"

namespace mm {

// what the fused loss (or the caller's dL/d rgba) contributes at one pixel
struct PixelLoss {
    float gin[3];       // the caller's dL/d colour (not fused; deferred fusion: the image's other consumers, or 0)
    float gi3[3];       // the masked ground-truth colours gt_c * gm + 1 * (1 - gm)
    float gmv;          // the ground-truth mask gm
    float kl1;          // fused: gs * image_weight / (B * 3 * H * W)
    float gsw, cnt;     // deferred: gs * image_weight and B * 3 * H * W, as recon_bwd_kernel forms them
};

// dL/d(colour c of this pixel) given its un-clamped value `pre`: the caller's gradient, or the fused loss's (the forward's clamp and
// masking expressions, shade_store / shade_empty_tiles + networks.py:370-377)
template <bool kDeferred>
__device__ inline float grad_colour(const PixelLoss& q, bool fused, int c, float pre) {
    if (!fused) return q.gin[c];
    const float pc = pre < 0.f ? 0.f : (pre > 1.f ? 1.f : pre);
    const float pi = pc * q.gmv + 1.f * (1.f - q.gmv);
    const float df = pi - q.gi3[c], sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
    if (kDeferred) return q.gsw * sg * q.gmv / q.cnt + q.gin[c];     // recon_bwd_kernel: gs * image_weight * sg * gm / cnt  (+ the caller's own gradient, 0 if none)
    return q.kl1 * sg * q.gmv;
}

// A pixel of a tile WITHOUT a covered pixel, no_mask: m = 0 and n = 0, so only the background and the two constant SH bands receive
// gradient.  coef = C0 * L0 + (0 - C6B) * L6.  Returns the pixel's dL/d(coef); gbg = its dL/dbg.
template <bool kDeferred>
__device__ inline float pixel_pass_background(const PixelLoss& q, bool fused, const float (&bgv)[3], float coef, float (&gbg)[3]) {
    float dc = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float pre = bgv[c] * coef;
        const float g = (pre >= 0.f && pre <= 1.f) ? grad_colour<kDeferred>(q, fused, c, pre) : 0.f;      // torch.clamp backward mask
        dc += g * bgv[c];
        gbg[c] = g * coef;
    }
    return dc;
}

// the forward quantities of one pixel of a tile with covered pixels, as shade_store forms them (uncovered lanes: zeros throughout)
struct PixelShade {
    int hf;                          // the winner, -1: uncovered
    float4 p0, p1;                   // its corners {ax,ay,bx,by} {cx,cy,..}
    float fu[6], n0, n1, n2;         // corner uvs, unit normal
    float w0, w1, w2, nrm, m;        // barycentrics, their padded sum, coverage (w0 + w1) + w2
    float nx, ny, nz;                // interpolated normal
    float x0, y0;                    // pixel centre
    float coef;                      // sum of bands x lights
};

struct PixelGrad {
    float dcs;                       // dL/d(coef): dL/dlights of the pixel = dcs * sh_bands(normal)
    float gbg[3];                    // dL/dbg (no_mask)
    float4 k0, k1; float k2;         // covered: the nine K2 numbers of the pixel's face
    float m2;                        // ... and their largest magnitude (0: uncovered)
    TexRecord rec;                   // the texture record, and the texture tiles under its footprint (-1: none)
    int rtile[4];
};

// tq: the twelve texels of the footprint (clamped addresses); L: lights in sh_bands' order
template <bool kNoMask, bool kDeferred>
__device__ inline void pixel_pass_shaded(const PixelLoss& q, bool fused, const PixelShade& h, const Bilin& s, const float (&tq)[3][4], const float (&L)[9],
                                         const float (&bgv)[3], int Ht, int Wt, int ntx, float mult, PixelGrad& o) {
    const bool inw = s.x0 < Wt && s.y0 < Ht, ine = s.x1 < Wt && s.y0 < Ht;
    const bool isw = s.x0 < Wt && s.y1 < Ht, ise = s.x1 < Wt && s.y1 < Ht;
    const float m = h.m, coef = h.coef, nx = h.nx, ny = h.ny, nz = h.nz;
    float dm = 0.f, dc = 0.f, gix = 0.f, giy = 0.f, dtcv[3];
    const float ex = 1.f - s.tx, ey = 1.f - s.ty;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float tnw = inw ? tq[c][0] : 0.f, tne = ine ? tq[c][1] : 0.f;
        const float tsw = isw ? tq[c][2] : 0.f, tse = ise ? tq[c][3] : 0.f;
        float tc = 0.f;
        if (inw) tc += tnw * s.wnw;
        if (ine) tc += tne * s.wne;
        if (isw) tc += tsw * s.wsw;
        if (ise) tc += tse * s.wse;
        float pre, dtc;
        if (kNoMask) {
            const float bgvc = bgv[c];
            const float base = tc * m + bgvc * (1.f - m);
            pre = base * coef;
            const float g = (pre >= 0.f && pre <= 1.f) ? grad_colour<kDeferred>(q, fused, c, pre) : 0.f;      // torch.clamp backward mask
            dc += g * base;
            const float dbase = g * coef;
            dtc = dbase * m;
            o.gbg[c] = dbase * (1.f - m);
            dm += dbase * (tc - bgvc);
        } else {
            pre = (tc * m) * coef + 1.f * (1.f - m);
            const float g = (pre >= 0.f && pre <= 1.f) ? grad_colour<kDeferred>(q, fused, c, pre) : 0.f;
            dc += g * (tc * m);
            dtc = (g * coef) * m;
            dm += g * (tc * coef - 1.f);
            o.gbg[c] = 0.f;
        }
        dtcv[c] = dtc;
        gix += dtc * ((tne - tnw) * ey + (tse - tsw) * s.ty);
        giy += dtc * ((tsw - tnw) * ex + (tse - tne) * s.tx);
    }
    o.dcs = dc;                                                  // dL/dlights = dc * bands(normal): formed at the end
    o.m2 = 0.f;
    o.rec.xy = 0; o.rec.tx = o.rec.ty = o.rec.d0 = o.rec.d1 = o.rec.d2 = 0.f;
    o.rtile[0] = o.rtile[1] = o.rtile[2] = o.rtile[3] = -1;
    if (h.hf >= 0) {
        const float w0 = h.w0, w1 = h.w1, w2 = h.w2, n0 = h.n0, n1 = h.n1, n2 = h.n2;
        const float4 p0 = h.p0, p1 = h.p1;
        const float x0 = h.x0, y0 = h.y0;
        const float* fu = h.fu;
        const float du = gix * s.mx * ((float)Wt / 2.f) * 2.f;
        const float dv = giy * s.my * ((float)Ht / 2.f) * -2.f;
        const float dnx = dc * (((MM_SH_C1 * L[1] + MM_SH_C4 * ny * L[4]) + MM_SH_C7 * nz * L[7]) + 2.f * MM_SH_C8 * nx * L[8]);
        const float dny = dc * (((MM_SH_C1 * L[3] + MM_SH_C4 * nx * L[4]) + MM_SH_C4 * nz * L[5]) - 2.f * MM_SH_C8 * ny * L[8]);
        const float dnz = dc * (((MM_SH_C1 * L[2] + MM_SH_C4 * ny * L[5]) + 2.f * MM_SH_C6 * nz * L[6]) + MM_SH_C7 * nx * L[7]);
        // K2 (Appendix A.1): this pixel's contribution to its face's corner and normal gradients; corner features are
        // (1, u_k, v_k, n).  Left per pixel; the face gather only has to add them up.
        const float gnn = (dnx * n0 + dny * n1) + dnz * n2;
        const float G0 = ((dm + du * fu[0]) + dv * fu[1]) + gnn;
        const float G1 = ((dm + du * fu[2]) + dv * fu[3]) + gnn;
        const float G2 = ((dm + du * fu[4]) + dv * fu[5]) + gnn;
        const float Gm = (w0 * G0 + w1 * G1) + w2 * G2;
        const float inrm = 1.f / h.nrm;
        const float dw0 = (G0 - Gm) * inrm, dw1 = (G1 - Gm) * inrm, dw2 = (G2 - Gm) * inrm;
        const float aex = p0.x - x0, aey = p0.y - y0, bex = p0.z - x0, bey = p0.w - y0, cex = p1.x - x0, cey = p1.y - y0;
        o.k0 = make_float4((dw1 * (-cey) + dw2 * bey) * mult, (dw1 * cex + dw2 * (-bex)) * mult,
                           (dw0 * cey + dw2 * (-aey)) * mult, (dw0 * (-cex) + dw2 * aex) * mult);
        o.k1 = make_float4((dw0 * (-bey) + dw1 * aey) * mult, (dw0 * bex + dw1 * (-aex)) * mult,
                           (w0 * dnx + w1 * dnx) + w2 * dnx, (w0 * dny + w1 * dny) + w2 * dny);
        o.k2 = (w0 * dnz + w1 * dnz) + w2 * dnz;
        const float4 k0 = o.k0, k1 = o.k1;
        o.m2 = fmaxf(fmaxf(fmaxf(fabsf(k0.x), fabsf(k0.y)), fmaxf(fabsf(k0.z), fabsf(k0.w))),
                     fmaxf(fmaxf(fmaxf(fabsf(k1.x), fabsf(k1.y)), fmaxf(fabsf(k1.z), fabsf(k1.w))), fabsf(o.k2)));
        if (dtcv[0] != 0.f || dtcv[1] != 0.f || dtcv[2] != 0.f) {
            o.rec.xy = (unsigned)s.x0 | ((unsigned)s.y0 << 16); o.rec.tx = s.tx; o.rec.ty = s.ty;
            o.rec.d0 = dtcv[0]; o.rec.d1 = dtcv[1]; o.rec.d2 = dtcv[2];
            // texture tiles under the bilinear footprint: up to 2x2 when it straddles a tile border
            const int tcx0 = s.x0 / MM_UV_TILE, tcy0 = s.y0 / MM_UV_TILE;
            const int tcx1 = (s.x1 < Wt ? s.x1 : s.x0) / MM_UV_TILE, tcy1 = (s.y1 < Ht ? s.y1 : s.y0) / MM_UV_TILE;
            o.rtile[0] = tcy0 * ntx + tcx0;
            o.rtile[1] = tcx1 != tcx0 ? tcy0 * ntx + tcx1 : -1;
            o.rtile[2] = tcy1 != tcy0 ? tcy1 * ntx + tcx0 : -1;
            o.rtile[3] = (tcx1 != tcx0 && tcy1 != tcy0) ? tcy1 * ntx + tcx1 : -1;
        }
    }
}

// The lanes of a wave that append to the same texture tile (rt; -1: none) form a group: its first lane is the group's leader, which takes the
// group's `size` consecutive slots with ONE returning atomic; a lane's slot is the leader's base + rank.  Pure lane arithmetic.
__device__ inline void tile_groups(int rt, int& leader, int& rank, int& size) {
    leader = -1; rank = 0; size = 0;
    unsigned long long pending = __ballot(rt >= 0);
    while (pending) {
        const int ld = __ffsll((unsigned long long)pending) - 1;
        const int tile = __builtin_amdgcn_readlane(rt, ld);      // (`ld` is wave-uniform: a scalar lane select, no LDS-crossbar round trip per tile)
        const unsigned long long m = __ballot(rt == tile);
        if (rt == tile) { leader = ld; rank = ballot_rank(m); size = __popcll(m); }
        pending &= ~m;
    }
}

// d lights of a wave's pixels: dl[i] = sum over the lanes of dcs * band_i(normal), fixed butterfly order, in the USER's light order
__device__ inline void wave_light_sums(bool any_covered, float dcs, float snx, float sny, float snz, int options, float (&dl)[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) dl[i] = 0.f;
    if (any_covered) {
        float bnd9[9];
        sh_bands(snx, sny, snz, bnd9);
#pragma unroll
        for (int i = 0; i < 9; ++i) dl[i] = wave_sum(dcs * bnd9[i]);
    } else { dl[0] = wave_sum(dcs * MM_SH_C0); dl[6] = wave_sum(dcs * (0.f - MM_SH_C6B)); }     // the other seven are zero
    if (options & MM_OPT_SH_ORDER_XYZ) { const float tmp = dl[2]; dl[2] = dl[3]; dl[3] = tmp; }   // back to the user's light order
}

}  // namespace mm
