// mm_pixel_bwd.hip -- pixel-major pass of the render path's backward for gfx950 (see mm_backward.hip for the scheme, mm_backward.h for why
// this half is compiled with the forward's floating-point flags).
#include "mm_backward.h"
#include "mm_pixel_pass.h"
#include "mm_plan.h"

namespace mm {

// ---------------------------------------------------------------------------------------------------------------------
// 1. pixel-major pass
// ---------------------------------------------------------------------------------------------------------------------
#ifndef MM_TOFF_SPIN_MAX
#define MM_TOFF_SPIN_MAX (1 << 12)   // polls of a tile's list offset (each a trip to memory: a few ms in all) before the lane forms the offset itself
#endif
#ifndef MM_PIXEL_LB
#define MM_PIXEL_LB 5             // waves per SIMD the register allocation is held to: 96 VGPRs without spills (the light gradients are carried as scalar + normal, not
#endif                            // as nine products); 5 workgroups of 28.9 KB LDS (the plan workgroups' staging) fit a CU as well
// kContour: the fused loss carries recon_data's contour term (MMRenderDesc.fused_contour > 0).  The reference's default is --lambda_contour 0
// (train.py:115, trainer.py:441): the default caller gets the instantiation without the term's code (24 vector instructions per wave and its
// registers), chosen by the host.
// kDeferred: DEFERRED fusion (BwdArgs::ltot as deferred_totals, MMRenderDesc.fused_totals): recon_data ran on its own on the image this render wrote; dL/d rgba is formed
// here with mm_recon_data_backward's expressions (csrc/mm_loss.hip: recon_bwd_kernel), in their order, from that call's per-image totals -- the bits
// that kernel would have written -- plus the caller's grad_rgba if there is one.  Never together with kContour.
// kViews: a multi-view call (BwdArgs::views > 1; never fused): bg, lights and textures are read from the image's SAMPLE (row b / views); what is
// written -- grad_bg included -- stays per image.  mm_render_backward launches the kViews = false instantiations, which hold none of that code.
// kIndexed: an indexed call (mm_render_indexed_backward; never fused, one view): bg, lights and textures are read from the image's rows in the plan's
// table, which travels in BwdArgs::ltot (indexed_table).  A trailing parameter: every other instantiation keeps its code.
template <bool kNoMask, bool kContour, bool kDeferred, bool kViews, bool kIndexed = false>
__global__ __launch_bounds__(256, MM_PIXEL_LB) void pixel_bwd_kernel(BwdArgs a) {
    __shared__ float s_dl[MM_BLOCK_WAVES][9];
    __shared__ float s_gm[MM_BLOCK_WAVES][2];
    if ((int)blockIdx.x < a.plan_wgs * a.B) {                    // (workgroup-uniform)
        __shared__ int s_wave[MM_PLAN_WGS][4];
        __shared__ unsigned short s_nch[MM_PLAN_LDS_FACES];
        plan_sweep_items<true>(a, blockIdx.x / a.plan_wgs, blockIdx.x % a.plan_wgs, s_wave, s_nch);
        return;
    }
    int b, blk;
    map_block(blockIdx.x - a.plan_wgs * a.B, a.B, a.blocks_per_image, b, blk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bx = blk % a.blocks_x, by = blk / a.blocks_x;
    const int px = bx * MM_BLOCK_PX + (wave & 1) * MM_TILE + (lane & 7), py = by * MM_BLOCK_PX + (wave >> 1) * MM_TILE + (lane >> 3);
    const bool in_img = px < a.W && py < a.H;
    const float x0 = pixel_x_k(px, a.W, a.kx), y0 = pixel_y_k(py, a.H, a.ky);                  // (host-formed IEEE quotients: the forward's centres)
    const size_t hw = (size_t)a.H * a.W, pin = (size_t)py * a.W + px;
    const size_t pix = (size_t)b * hw + pin;
    const int sb = kViews ? b / a.views : b;                      // the row of the per-sample inputs
    const int sb_t = kIndexed ? index_row(indexed_table(a), a.B, MM_IX_TEXTURES, b) : sb;
    const int sb_l = kIndexed ? index_row(indexed_table(a), a.B, MM_IX_LIGHTS, b) : sb;
    const int sb_g = kIndexed ? index_row(indexed_table(a), a.B, MM_IX_BG, b) : sb;
    if (blk == 0 && threadIdx.x == 0) a.ticket[b] = 0u;           // arrival counter of the vertex backward, used after this kernel
    // The pass is a chain of dependent trips to memory; it is written so that four remain: (1) everything addressed by the pixel
    // alone -- face_idx, prediction, ground truth, background; (2) what the winner's id addresses -- geometry, normal, corner uvs;
    // (3) the twelve texels, unconditionally from clamped addresses; (4) the record-slot atomics.  (Loads left inside per-lane
    // branches or behind stores that might alias them each cost the wave a trip of their own.)
    float bgv[3] = {0.f, 0.f, 0.f};
    if (kNoMask && in_img) {
#pragma unroll
        for (int c = 0; c < 3; ++c) bgv[c] = a.bg[((size_t)sb_g * 3 + c) * hw + pin];
    }
    float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f);
    int hf = -1;
    // fused recon_data backward (Appendix A.4): dL/dpred_c = kl1 * sign(pred_c' - gt_c') * gm needs the PREDICTION -- which this pass
    // recomputes anyway, bit for bit (it is compiled like the forward for that reason: mm_backward.h), so the forward image is not read
    // back (16 bytes per pixel of a bandwidth-bound kernel); the sign is taken where the pixel's colour is re-formed (grad_colour below).
    PixelLoss pl;                                                // (mm_pixel_pass.h)
    float (&gi3)[3] = pl.gi3;
    float &gmv = pl.gmv, &kl1 = pl.kl1, &gsw = pl.gsw, &cnt = pl.cnt;   // kDeferred: gs * image_weight and B*3*H*W, as recon_bwd_kernel forms them
    gi3[0] = gi3[1] = gi3[2] = 0.f; gmv = 0.f; kl1 = 0.f; gsw = 0.f; cnt = 1.f;
    const bool fused = a.gt != nullptr;
    if (kDeferred) {
        const float gs = a.grad_loss ? a.grad_loss[0] : 1.f;
        gsw = gs * a.image_weight;
        cnt = (float)a.B * 3.f * (float)a.H * (float)a.W;
        const float up = deferred_totals(a)[b * 4 + 1], U = deferred_totals(a)[b * 4 + 2] + 1e-10f;
        if (in_img) {
            hf = a.face_idx[pix];
            const float* g = a.gt + (size_t)b * 4 * hw;
            const float gm = g[3 * hw + pin];
            gmv = gm;
#pragma unroll
            for (int c = 0; c < 3; ++c) gi3[c] = g[c * hw + pin] * gm + 1.f * (1.f - gm);
            g4.w = gs * (-(1.f / (float)a.B) * (gm / U - up * (1.f - gm) / (U * U)));
            if (a.grad_rgba) {                                   // the image's other consumers (autograd would have added the two gradients)
                const float4 ext = *(const float4*)(a.grad_rgba + pix * 4);
                g4.x = ext.x; g4.y = ext.y; g4.z = ext.z; g4.w += ext.w;
            }
        }
    } else if (fused) {
        // the image's totals are exact integer sums left by its raster waves
        float l1s, up, un;
        loss_totals(a.ltot, b, l1s, up, un);
        const float U = un + 1e-10f;
        const float gs = a.grad_loss ? a.grad_loss[0] : 1.f;
        // everything that is the same for all pixels of the image is folded into three coefficients (wave-uniform arithmetic
        // once, instead of four divisions per lane): dL/dpred_c = kl1 * sign * gm,  dL/dalpha = ka * gm + kb * (1 - gm)
        kl1 = gs * a.image_weight / ((float)a.B * 3.f * (float)a.H * (float)a.W);
        const float ka = -gs / ((float)a.B * U), kb = gs * up / ((float)a.B * U * U);
        if (in_img) {
            hf = a.face_idx[pix];
            const float* g = a.gt + (size_t)b * 4 * hw;
            const float gm = g[3 * hw + pin];
            gmv = gm;
#pragma unroll
            for (int c = 0; c < 3; ++c) gi3[c] = g[c * hw + pin] * gm + 1.f * (1.f - gm);
            g4.w = ka * gm + kb * (1.f - gm);
        }
        if (kContour) {                                          // the contour term, networks.py:379-388 (forward: contour_term, mm_raster_common.h)
            // d/dalpha of  kc * sum_p (|alpha_p - alpha_s(p)| - |gm_p - gm_s(p)|)^2,  s(p) = top-left pixel of p's 4x4 block = lane (lane & 0x24) of this
            // wave: pixel p gets +g_p, its block's corner pixel -sum of the block's g (its own g is 0: |0| has gradient 0, as torch.abs has).
            // alpha is re-formed from the saved soft-mask state exactly as shade_store formed it: covered 1, else 1 - keepprod.
            const float kc = gs * a.contour / ((float)a.B * (float)a.H * (float)a.W);
            float al = 0.f;
            if (in_img) { const float sx = a.soft[pix].x; al = hf >= 0 ? 1.f : 1.f - (sx > 0.f ? sx : 0.f); }
            const int src = lane & 0x24;
            const float as = __shfl(al, src, 64), gms = __shfl(gmv, src, 64);
            float gc = 0.f;
            if (in_img) {
                const float dd = al - as, cp = fabsf(dd), cg = fabsf(gmv - gms);
                gc = (kc * 2.f * (cp - cg)) * (dd > 0.f ? 1.f : (dd < 0.f ? -1.f : 0.f));
            }
            float bs = gc;                                       // the 4x4 block's sum, fixed order: columns (lane bits 0, 1), then rows (bits 3, 4)
            bs += __shfl_xor(bs, 1, 64); bs += __shfl_xor(bs, 2, 64); bs += __shfl_xor(bs, 8, 64); bs += __shfl_xor(bs, 16, 64);
            if (in_img) g4.w += lane == src ? -bs : gc;
        }
    } else if (in_img) { g4 = *(const float4*)(a.grad_rgba + pix * 4); hf = a.face_idx[pix]; }
    pl.gin[0] = g4.x; pl.gin[1] = g4.y; pl.gin[2] = g4.z;
    // (dL/d colour from the un-clamped value, the K2 numbers, the texture record: mm_pixel_pass.h, one text with the forward's step-mode epilogue)
    float m2 = 0.f, m4 = 0.f;                                    // this lane's largest |K2 number| / |dL/dalpha|: the gather's fixed-point scale
    if (in_img && hf < 0) { a.gp2[pix] = g4.w; m4 = fabsf(g4.w); }   // the face gather (K4) needs dL/dalpha of uncovered pixels
    // dL/dlights of this pixel = dcs * sh_bands(normal): kept as the scalar and the normal (4 registers, not 9, across the record append below)
    float dcs = 0.f, snx = 0.f, sny = 0.f, snz = 0.f;
    TexRecord rec; rec.xy = 0; rec.tx = rec.ty = rec.d0 = rec.d1 = rec.d2 = 0.f;
    int rtile[4] = {-1, -1, -1, -1};

    // Tiles without a covered pixel (more than half of them): m = 0 and n = 0 in every lane, so only the background and the two
    // constant SH bands receive gradient -- none of the uv / bilinear / texel / barycentric work below is needed.
    const bool any_covered = __ballot(in_img && hf >= 0) != 0;   // wave-uniform
    if (!any_covered) {
        if (kNoMask && in_img) {
            const float* L = a.lights + sb_l * 9;                 // (bands 0 and 6 only: the same lights whatever the band order)
            const float coef = MM_SH_C0 * L[0] + (0.f - MM_SH_C6B) * L[6];
            float gbg[3];
            dcs = pixel_pass_background<kDeferred>(pl, fused, bgv, coef, gbg);      // (normal 0: bands 0 and 6 only)
#pragma unroll
            for (int c = 0; c < 3; ++c) a.grad_bg[((size_t)b * 3 + c) * hw + pin] = gbg[c];
        }
    } else if (in_img && (hf >= 0 || kNoMask)) {
        // recompute the forward quantities of this pixel (only face_idx and the soft-mask state were saved)
        float w0 = 0.f, w1 = 0.f, w2 = 0.f, nrm = 1.f, m = 0.f, u = 0.f, v = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
        float fu[6] = {0, 0, 0, 0, 0, 0}, n0 = 0.f, n1 = 0.f, n2 = 0.f;
        float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0;
        {   // trip 2 (uncovered lanes of a covered tile read face 0's records and ignore them)
            const int fs = max(hf, 0);
            const float4* geo = a.geo + ((size_t)b * a.F + fs) * 3;
            const float4 q0 = geo[0], q1 = geo[1];
            const float2* fuv = (const float2*)(a.face_uvs + (size_t)fs * 6);
            const float2 u0 = fuv[0], u1 = fuv[1], u2 = fuv[2];
            const float* nn = a.fn + ((size_t)b * a.F + fs) * 3;
            const float m0 = nn[0], m1 = nn[1], m2 = nn[2];
            if (hf >= 0) {
                p0 = q0; p1 = q1;
                fu[0] = u0.x; fu[1] = u0.y; fu[2] = u1.x; fu[3] = u1.y; fu[4] = u2.x; fu[5] = u2.y;
                n0 = m0; n1 = m1; n2 = m2;
            }
        }
        if (hf >= 0) {
            // (MM_OPT_BARY_ONE_MINUS changes the weights by O(eps); the derivative below stays that of the default form)
            bary_weights(p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, x0, y0, a.eps, (a.options & MM_OPT_BARY_ONE_MINUS) != 0, w0, w1, w2, nrm);
            m = (w0 + w1) + w2;
            u = (w0 * fu[0] + w1 * fu[2]) + w2 * fu[4];
            v = (w0 * fu[1] + w1 * fu[3]) + w2 * fu[5];
            nx = (w0 * n0 + w1 * n0) + w2 * n0;
            ny = (w0 * n1 + w1 * n1) + w2 * n1;
            nz = (w0 * n2 + w1 * n2) + w2 * n2;
        }
        const Bilin s = bilin_setup(u, v, a.Ht, a.Wt);
        // trip 3: twelve loads in flight together
        float tq[3][4];
        {
            const int cx0 = min(max(s.x0, 0), a.Wt - 1), cx1 = min(max(s.x1, 0), a.Wt - 1);
            const int cy0 = min(max(s.y0, 0), a.Ht - 1), cy1 = min(max(s.y1, 0), a.Ht - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* tex = a.textures + ((size_t)sb_t * 3 + c) * a.Ht * a.Wt;
                tq[c][0] = tex[(size_t)cy0 * a.Wt + cx0]; tq[c][1] = tex[(size_t)cy0 * a.Wt + cx1];
                tq[c][2] = tex[(size_t)cy1 * a.Wt + cx0]; tq[c][3] = tex[(size_t)cy1 * a.Wt + cx1];
            }
        }
        float bnd[9];
        sh_bands(nx, ny, nz, bnd);
        float L[9];                                              // lights in sh_bands' order (see shade_store)
#pragma unroll
        for (int i = 0; i < 9; ++i) L[i] = a.lights[sb_l * 9 + i];
        if (a.options & MM_OPT_SH_ORDER_XYZ) { const float tmp = L[2]; L[2] = L[3]; L[3] = tmp; }
        float coef = 0.f;
#pragma unroll
        for (int i = 0; i < 9; ++i) coef += bnd[i] * L[i];

        PixelShade sh;
        sh.hf = hf; sh.p0 = p0; sh.p1 = p1; sh.n0 = n0; sh.n1 = n1; sh.n2 = n2;
#pragma unroll
        for (int i = 0; i < 6; ++i) sh.fu[i] = fu[i];
        sh.w0 = w0; sh.w1 = w1; sh.w2 = w2; sh.nrm = nrm; sh.m = m; sh.nx = nx; sh.ny = ny; sh.nz = nz; sh.x0 = x0; sh.y0 = y0; sh.coef = coef;
        PixelGrad pg;
        pixel_pass_shaded<kNoMask, kDeferred>(pl, fused, sh, s, tq, L, bgv, a.Ht, a.Wt, a.ntx, a.mult, pg);
        if (kNoMask) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.grad_bg[((size_t)b * 3 + c) * hw + pin] = pg.gbg[c];
        }
        dcs = pg.dcs; snx = nx; sny = ny; snz = nz;              // dL/dlights = dc * bands(normal): formed at the end
        if (hf >= 0) { a.gp[pix * 2 + 0] = pg.k0; a.gp[pix * 2 + 1] = pg.k1; a.gp2[pix] = pg.k2; m2 = pg.m2; }
        rec = pg.rec;
#pragma unroll
        for (int c = 0; c < 4; ++c) rtile[c] = pg.rtile[c];
    }
    // append the records: one returning atomic per (wave, distinct tile), lanes of the same tile take consecutive slots of the tile's list, which
    // starts at the tile's offset in the image's packed record array -- read by the group's leader in the same trip as its atomic (written by the
    // image's plan workgroup at the top of its life, + 1: a zero means "not yet", the first microseconds of the launch, and is asked for again).
    // The grouping is pure lane arithmetic; all leaders then issue their atomics in ONE instruction per footprint corner (and the four corners'
    // atomics are in flight together), so a wave pays one fabric round trip, not one per tile.
    int leader[4], rank[4], base[4], toff[4], room[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        leader[c] = -1; rank[c] = 0; base[c] = 0; toff[c] = 1; room[c] = 0;
        if (!any_covered) continue;                              // wave-uniform: nothing to append
        int size;
        tile_groups(rtile[c], leader[c], rank[c], size);
        if (leader[c] == lane) {
            toff[c] = __hip_atomic_load(a.toff + (size_t)b * a.ntiles_ + rtile[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            room[c] = a.trcnt[(size_t)b * a.ntiles_ + rtile[c]];    // what the forward counted for this tile: the length of its list
            base[c] = atomicAdd(a.tcur + (size_t)b * a.ntiles_ + rtile[c], size);
        }
    }
    // (the slots are on their way: the wave's light-gradient sums are formed meanwhile, the records stored after them)
    // d lights: wave butterfly -> one LDS row per wave -> fixed-order partial of this workgroup (summed by vertex_bwd)
    float dl[9];
    wave_light_sums(any_covered, dcs, snx, sny, snz, a.options, dl);
    m2 = wave_max(m2); m4 = wave_max(m4);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) s_dl[wave][i] = dl[i];
        s_gm[wave][0] = m2; s_gm[wave][1] = m4;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!any_covered) break;
        // (the image's plan workgroup has a LOWER workgroup index and writes the offsets first thing: it is in flight before this wave exists,
        //  and the wait below is the first microseconds of a launch.  Progress does NOT depend on that order: the offset is a pure function of
        //  the forward's per-tile counts, which are complete before this launch -- should it not arrive within the bound (a dispatcher that
        //  does not start workgroups in index order, CU masking, a debugger), the lane adds the counts up itself: the same number, later.)
        int spins = 0;
        while (__builtin_expect(leader[c] == lane && toff[c] == 0, 0)) {
            if (++spins > MM_TOFF_SPIN_MAX) {
                const int* cnt = a.trcnt + (size_t)b * a.ntiles_;
                int run = 1;                                     // (stored + 1, as the plan workgroup stores it)
                for (int t = 0; t < rtile[c]; ++t) run += cnt[t];
                toff[c] = run;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
            toff[c] = __hip_atomic_load(a.toff + (size_t)b * a.ntiles_ + rtile[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        room[c] = toff[c] == 0 ? 0 : room[c] - base[c];           // places left in the tile's list from this group's first one (<= 0: none)
        base[c] += toff[c] - 1;
    }
    int ndrop = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!any_covered) break;
        const int bs = __shfl(base[c], leader[c] < 0 ? lane : leader[c], 64), rm = __shfl(room[c], leader[c] < 0 ? lane : leader[c], 64);
        if (rtile[c] >= 0) {
            const int pos = bs + rank[c];
            // inside the image's array AND inside the tile's own list (the forward's count is an upper bound of what this pass appends as
            // long as both recompute the same footprints; a record beyond it would land in the NEXT tile's list: dropped and reported instead)
            if (pos < a.trcap && rank[c] < rm) a.trec[(size_t)b * a.trcap + pos] = rec;
            else ++ndrop;                                        // counted, and the texture gather poisons the image's gradient
        }
    }
    if (__builtin_expect(__ballot(ndrop != 0) != 0ull, 0)) { if (ndrop) atomicAdd(a.tdrop + b, ndrop); }

    __syncthreads();
    if (threadIdx.x >= 64 && threadIdx.x < 66) {                 // non-negative floats order like their bit patterns: integer max, one atomic per
        const int k = threadIdx.x - 64;                          // workgroup and kind (NaN / inf gradients end up as an inf scale = zero sums)
        const float m = fmaxf(fmaxf(s_gm[0][k], s_gm[1][k]), fmaxf(s_gm[2][k], s_gm[3][k]));
        // one atomic per workgroup and kind, spread over MM_GSHARD words per image on separate 32-byte sectors (thousands of
        // workgroups per image on ONE word queue at the memory side: measured +75 % on this kernel at 512x512)
        if (m > 0.f) atomicMax(a.gmax + ((size_t)b * MM_GSHARD + (blk & (MM_GSHARD - 1))) * 8 + k, __float_as_uint(m));
    }
    if (threadIdx.x < 9)
        a.dl_part[((size_t)b * a.blocks_per_image + blk) * 12 + threadIdx.x] =
            ((s_dl[0][threadIdx.x] + s_dl[1][threadIdx.x]) + s_dl[2][threadIdx.x]) + s_dl[3][threadIdx.x];
}

int launch_pixel_bwd(const BwdArgs& a, const MMRenderDesc* d, hipStream_t s) {
    ProfScope p(d->prof_events, MM_PROF_PIXEL_BWD, s);
    dim3 grid(a.blocks_per_image * d->B + a.plan_wgs * d->B);    // + the plan workgroups, in front
    const bool contour = a.gt != nullptr && a.contour > 0.f;
    if (a.views == 0) {                                          // indexed (BwdArgs::views; never fused: mm_render_indexed_backward refuses it)
        if (d->no_mask) hipLaunchKernelGGL((pixel_bwd_kernel<true, false, false, false, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((pixel_bwd_kernel<false, false, false, false, true>), grid, dim3(256), 0, s, a);
        return MM_OK;
    }
    if (a.views > 1) {                                           // multi-view (never fused: mm_render_views_backward refuses it)
        if (d->no_mask) hipLaunchKernelGGL((pixel_bwd_kernel<true, false, false, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((pixel_bwd_kernel<false, false, false, true>), grid, dim3(256), 0, s, a);
        return MM_OK;
    }
    if (a.options & MM_INT_DEFERRED) {                           // deferred fusion (never with the contour term: check_render)
        if (d->no_mask) hipLaunchKernelGGL((pixel_bwd_kernel<true, false, true, false>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((pixel_bwd_kernel<false, false, true, false>), grid, dim3(256), 0, s, a);
        return MM_OK;
    }
    if (d->no_mask) { if (contour) hipLaunchKernelGGL((pixel_bwd_kernel<true, true, false, false>), grid, dim3(256), 0, s, a); else hipLaunchKernelGGL((pixel_bwd_kernel<true, false, false, false>), grid, dim3(256), 0, s, a); }
    else { if (contour) hipLaunchKernelGGL((pixel_bwd_kernel<false, true, false, false>), grid, dim3(256), 0, s, a); else hipLaunchKernelGGL((pixel_bwd_kernel<false, false, false, false>), grid, dim3(256), 0, s, a); }
    return MM_OK;
}

}  // namespace mm
