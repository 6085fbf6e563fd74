// mm_ssim.hip -- pytorch_msssim's SSIM (the reference's evaluation metric, trainer.py:771-795, 911-935; test.py:428-457) for gfx950.
//
// Upstream is ten grouped F.conv2d calls and about twenty elementwise / reduction kernels per call.  Here:
//   forward   ssim_tile_kernel<false>: one 256-thread workgroup per 64x16 output tile of one (n, c) plane stages the tile's input halo of
//             X and Y in LDS, filters the five moments (x, y, x^2, y^2, xy) one at a time -- vertical pass into LDS, horizontal pass into
//             registers --, evaluates ssim_map and cs_map per pixel and writes the tile's two partial sums.  No moment or map goes to HBM.
//             ssim_fold_kernel: one workgroup sums every plane's tile partials in a fixed order and writes ssim / cs per channel and the
//             requested means.  2 launches.
//   backward  ssim_tile_kernel<true>: the same tile pass recomputes the moments and writes the adjoint maps
//             a_m = (g_ssim dS/dm + g_cs dcs/dm) / P, m in {mx, my, Exx, Eyy, Exy}, into the workspace (four maps: a_Exx = a_Eyy);
//             ssim_gather_kernel: per 64x16 INPUT tile, the adjoint of the valid filter (a zero-padded full correlation with the reversed
//             taps, written as a gather) of each map, then dX = G'a_mx + 2x G'a_xx + y G'a_xy, dY = G'a_my + 2y G'a_yy + x G'a_xy.
//             2 launches.
// No float atomics anywhere: every sum has a fixed order, so results are bitwise reproducible, and a plane's values depend on that plane
// alone (an image's result does not depend on the rest of the batch).
//
// LDS per workgroup, Cw = 64 + kw - 1 columns: forward / adjoint (2 (16 + kh - 1) + 16) Cw floats (19.7 KiB at win 11, 39.7 KiB at win 31),
// gather ((16 + kh - 1) + 16) Cw floats (12.1 / 22.8 KiB): at least three workgroups per CU at every window size.
#include "mm_device.h"

#define SS_TW 64            // output tile columns (one wave's lanes)
#define SS_TH 16            // output tile rows (four per wave)
#define SS_THREADS 256
#define SS_MAPS 4           // adjoint maps of the backward: mx, my, Exx (= Eyy: D depends on both alike), Exy

namespace mm {

// the separable window as the kernels use it: kh / kw taps along H / W (1 and a tap of 1 along a dimension the skip rule leaves alone)
struct SsimFilter {
    int N, C, H, W, Ho, Wo, kh, kw;
    int ntx, nty;           // tiles per plane (of the output extent for the tile kernel, of the input extent for the gather)
    float vt[MM_SSIM_MAX_WIN], ht[MM_SSIM_MAX_WIN];
};

struct SsimIn {
    const float* p;
    int64_t s[4];
    __device__ float at(int n, int c, int h, int w) const {
        return p[(int64_t)n * s[0] + (int64_t)c * s[1] + (int64_t)h * s[2] + (int64_t)w * s[3]];
    }
};

template <int M> __device__ inline float ssim_moment(float x, float y) {
    MM_FP_EXACT
    return M == 0 ? x : M == 1 ? y : M == 2 ? x * x : M == 3 ? y * y : x * y;
}

// vertical pass of moment M over the staged halo (rows of Cw floats) into sv (SS_TH rows), then the horizontal pass of this thread's four
// pixels (column tid & 63, rows (tid >> 6) + 4j) into acc.  Two barriers: sv is free again when it returns.
template <int M>
__device__ inline void ssim_filter_moment(const float* sx, const float* sy, float* sv, int Cw, const SsimFilter& f, float acc[4]) {
    MM_FP_EXACT
    const int tid = threadIdx.x;
    for (int i = tid; i < SS_TH * Cw; i += SS_THREADS) {
        const int r = i / Cw, c = i - r * Cw;
        float a = 0.f;
        for (int t = 0; t < f.kh; ++t) {
            const int o = (r + t) * Cw + c;
            a += f.vt[t] * ssim_moment<M>(sx[o], M == 0 || M == 2 ? 0.f : sy[o]);
        }
        sv[i] = a;
    }
    __syncthreads();
    const int c = tid & 63;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float* row = sv + ((tid >> 6) + 4 * j) * Cw + c;
        float a = 0.f;
        for (int t = 0; t < f.kw; ++t) a += f.ht[t] * row[t];
        acc[j] = a;
    }
    __syncthreads();
}

// ---- forward tile pass (BWD = false) / adjoint maps of the backward (BWD = true) ------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(SS_THREADS) void ssim_tile_kernel(SsimIn X, SsimIn Y, SsimFilter f, float C1, float C2, float* partial,
                                                               const float* g_ssim, const float* g_cs, float* adj) {
    MM_FP_EXACT
    extern __shared__ float smem[];
    __shared__ float red[SS_THREADS / 64][2];
    const int ntiles = f.ntx * f.nty;
    const int plane = blockIdx.x / ntiles, tile = blockIdx.x - plane * ntiles;
    const int n = plane / f.C, ch = plane - n * f.C;
    const int oy0 = (tile / f.ntx) * SS_TH, ox0 = (tile % f.ntx) * SS_TW;
    const int R = SS_TH + f.kh - 1, Cw = SS_TW + f.kw - 1;
    float* sx = smem;
    float* sy = sx + R * Cw;
    float* sv = sy + R * Cw;
    const int tid = threadIdx.x;
    // the halo of the tile; outside the image (only under outputs past Ho / Wo, which are masked below) reads as 0
    for (int i = tid; i < R * Cw; i += SS_THREADS) {
        const int r = i / Cw, c = i - r * Cw;
        const int gy = oy0 + r, gx = ox0 + c;
        const bool in = gy < f.H && gx < f.W;
        sx[i] = in ? X.at(n, ch, gy, gx) : 0.f;
        sy[i] = in ? Y.at(n, ch, gy, gx) : 0.f;
    }
    __syncthreads();
    float mx[4], my[4], exx[4], eyy[4], exy[4];
    ssim_filter_moment<0>(sx, sy, sv, Cw, f, mx);
    ssim_filter_moment<1>(sx, sy, sv, Cw, f, my);
    ssim_filter_moment<2>(sx, sy, sv, Cw, f, exx);
    ssim_filter_moment<3>(sx, sy, sv, Cw, f, eyy);
    ssim_filter_moment<4>(sx, sy, sv, Cw, f, exy);

    const int ox = ox0 + (tid & 63);
    const float P = (float)f.Ho * (float)f.Wo;
    float gs = 0.f, gc = 0.f;
    if (BWD) {
        gs = g_ssim ? g_ssim[plane] / P : 0.f;
        gc = g_cs ? g_cs[plane] / P : 0.f;
    }
    float s_sum = 0.f, c_sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int oy = oy0 + (tid >> 6) + 4 * j;
        if (oy >= f.Ho || ox >= f.Wo) continue;
        // upstream's expressions in upstream's order (pytorch_msssim._ssim)
        const float m1s = mx[j] * mx[j], m2s = my[j] * my[j], m12 = mx[j] * my[j];
        const float s1 = exx[j] - m1s, s2 = eyy[j] - m2s, s12 = exy[j] - m12;
        const float Cn = 2.f * s12 + C2, D = s1 + s2 + C2;
        const float A = 2.f * m12 + C1, B = m1s + m2s + C1;
        const float cs = Cn / D, L = A / B;
        const float S = L * cs;
        if (!BWD) {
            s_sum += S;
            c_sum += cs;
        } else {
            // dS/dm and dcs/dm; dL/dmx = L (2my/A - 2mx/B) is written as (2my - 2mx L)/B: no division by A, which vanishes for signed inputs
            const float dcs_dxx = -cs / D, dcs_dxy = 2.f / D;
            const float dcs_dmx = (2.f * mx[j] * cs - 2.f * my[j]) / D, dcs_dmy = (2.f * my[j] * cs - 2.f * mx[j]) / D;
            const float dL_dmx = (2.f * my[j] - 2.f * mx[j] * L) / B, dL_dmy = (2.f * mx[j] - 2.f * my[j] * L) / B;
            const float a_mx = gs * (cs * dL_dmx + L * dcs_dmx) + gc * dcs_dmx;
            const float a_my = gs * (cs * dL_dmy + L * dcs_dmy) + gc * dcs_dmy;
            const float a_ee = gs * (L * dcs_dxx) + gc * dcs_dxx;       // dS/dExx = L dcs/dExx = -S/D, and the same for Eyy
            const float a_xy = gs * (L * dcs_dxy) + gc * dcs_dxy;
            const size_t P64 = (size_t)f.Ho * f.Wo;
            float* a = adj + (size_t)plane * SS_MAPS * P64 + (size_t)oy * f.Wo + ox;
            a[0] = a_mx; a[P64] = a_my; a[2 * P64] = a_ee; a[3 * P64] = a_xy;
        }
    }
    if (BWD) return;
    // (not block_sum_wide: this tile sum adds its waves as a tree, (w0 + w1) + (w2 + w3), and the SSIM values are pinned to that order)
    s_sum = wave_sum(s_sum);
    c_sum = wave_sum(c_sum);
    if ((tid & 63) == 0) { red[tid >> 6][0] = s_sum; red[tid >> 6][1] = c_sum; }
    __syncthreads();
    if (tid < 2) partial[(size_t)blockIdx.x * 2 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// nonnegative_ssim's relu as torch.relu computes it: a negative value becomes 0 and a NaN (a diverged render) stays NaN -- fmaxf would
// return the 0 and score the plane a silent 0
__device__ inline float ssim_relu(float v, int nonneg) { return (nonneg && v < 0.f) ? 0.f : v; }

// ---- forward fold: one workgroup, every sum in a fixed order ------------------------------------------------------------------
__global__ __launch_bounds__(1024) void ssim_fold_kernel(const float* partial, int planes, int ntiles, int C, float P, int nonneg,
                                                         float* ssim, float* cs, float* mean_c, float* mean_all) {
    MM_FP_EXACT
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int p = wave; p < planes; p += 16) {
        float s = 0.f, c = 0.f;
        for (int i = lane; i < ntiles; i += 64) {
            s += partial[((size_t)p * ntiles + i) * 2];
            c += partial[((size_t)p * ntiles + i) * 2 + 1];
        }
        s = wave_sum(s);
        c = wave_sum(c);
        if (lane == 0) {
            ssim[p] = s / P;
            if (cs) cs[p] = c / P;
        }
    }
    if (!mean_c && !mean_all) return;
    __syncthreads();                                    // (workgroup scope: this workgroup's ssim[] stores are visible to it)
    if (mean_c) {
        const int Nimg = planes / C;
        for (int n = tid; n < Nimg; n += 1024) {
            float s = 0.f;
            for (int c = 0; c < C; ++c) {
                const float v = ssim[(size_t)n * C + c];
                s += ssim_relu(v, nonneg);
            }
            mean_c[n] = s / (float)C;
        }
    }
    if (mean_all && wave == 0) {
        float s = 0.f;
        for (int p = lane; p < planes; p += 64) {
            const float v = ssim[p];
            s += ssim_relu(v, nonneg);
        }
        s = wave_sum(s);
        if (lane == 0) mean_all[0] = s / (float)planes;
    }
}

// ---- backward gather: the adjoint of the valid separable filter, per 64x16 input tile ------------------------------------------
// f.vt / f.ht hold the REVERSED taps: x_grad[i] = sum_s g[k-1-s] a[i-(k-1)+s] over the maps zero-padded by k-1 on each side.
__global__ __launch_bounds__(SS_THREADS) void ssim_gather_kernel(SsimIn X, SsimIn Y, SsimFilter f, const float* adj, float* gx, float* gy) {
    MM_FP_EXACT
    extern __shared__ float smem[];
    const int ntiles = f.ntx * f.nty;
    const int plane = blockIdx.x / ntiles, tile = blockIdx.x - plane * ntiles;
    const int n = plane / f.C, ch = plane - n * f.C;
    const int iy0 = (tile / f.ntx) * SS_TH, ix0 = (tile % f.ntx) * SS_TW;
    const int R = SS_TH + f.kh - 1, Cw = SS_TW + f.kw - 1;
    const int ay0 = iy0 - (f.kh - 1), ax0 = ix0 - (f.kw - 1);
    float* sa = smem;
    float* sv = sa + R * Cw;
    const int tid = threadIdx.x;
    const size_t P64 = (size_t)f.Ho * f.Wo;
    float g[SS_MAPS][4];
#pragma unroll
    for (int m = 0; m < SS_MAPS; ++m) {
        const float* a = adj + ((size_t)plane * SS_MAPS + m) * P64;
        for (int i = tid; i < R * Cw; i += SS_THREADS) {
            const int r = i / Cw, c = i - r * Cw;
            const int y = ay0 + r, x = ax0 + c;
            sa[i] = (y >= 0 && y < f.Ho && x >= 0 && x < f.Wo) ? a[(size_t)y * f.Wo + x] : 0.f;
        }
        __syncthreads();
        ssim_filter_moment<0>(sa, sa, sv, Cw, f, g[m]);
    }
    const int x = ix0 + (tid & 63);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = iy0 + (tid >> 6) + 4 * j;
        if (y >= f.H || x >= f.W) continue;
        const float xv = X.at(n, ch, y, x), yv = Y.at(n, ch, y, x);
        const size_t o = (size_t)plane * f.H * f.W + (size_t)y * f.W + x;
        if (gx) gx[o] = g[0][j] + 2.f * xv * g[2][j] + yv * g[3][j];
        if (gy) gy[o] = g[1][j] + 2.f * yv * g[2][j] + xv * g[3][j];
    }
}

static SsimFilter make_filter(const MMSsimDesc* d, bool output_tiles, bool reversed) {
    SsimFilter f;
    f.N = d->N; f.C = d->C; f.H = d->H; f.W = d->W;
    const int k = d->win_size;
    f.kh = d->H >= k ? k : 1;               // upstream's skip rule: a dimension shorter than the window is not filtered
    f.kw = d->W >= k ? k : 1;
    f.Ho = d->H - f.kh + 1;
    f.Wo = d->W - f.kw + 1;
    for (int t = 0; t < MM_SSIM_MAX_WIN; ++t) f.vt[t] = f.ht[t] = 0.f;
    for (int t = 0; t < f.kh; ++t) f.vt[t] = f.kh == 1 ? 1.f : d->win[reversed ? k - 1 - t : t];
    for (int t = 0; t < f.kw; ++t) f.ht[t] = f.kw == 1 ? 1.f : d->win[reversed ? k - 1 - t : t];
    const int eh = output_tiles ? f.Ho : f.H, ew = output_tiles ? f.Wo : f.W;
    f.ntx = (ew + SS_TW - 1) / SS_TW;
    f.nty = (eh + SS_TH - 1) / SS_TH;
    return f;
}

static size_t tile_lds_bytes(const SsimFilter& f, int staged) {
    return (size_t)(staged * (SS_TH + f.kh - 1) + SS_TH) * (SS_TW + f.kw - 1) * sizeof(float);
}

size_t ssim_workspace_bytes(const MMSsimDesc* d) {
    const SsimFilter f = make_filter(d, true, false);
    const size_t planes = (size_t)d->N * d->C;
    const size_t fwd = planes * f.ntx * f.nty * 2 * sizeof(float);
    const size_t bwd = planes * SS_MAPS * (size_t)f.Ho * f.Wo * sizeof(float);
    return align256(fwd > bwd ? fwd : bwd);
}

static SsimIn in_of(const float* p, const int64_t* s) {
    SsimIn r;
    r.p = p;
    for (int i = 0; i < 4; ++i) r.s[i] = s[i];
    return r;
}

int launch_ssim_fwd(const MMSsimDesc* d, hipStream_t stream) {
    const SsimFilter f = make_filter(d, true, false);
    const int planes = d->N * d->C, ntiles = f.ntx * f.nty;
    float* partial = (float*)d->workspace;
    hipLaunchKernelGGL(ssim_tile_kernel<false>, dim3(planes * ntiles), dim3(SS_THREADS), tile_lds_bytes(f, 2), stream,
                       in_of(d->x, d->x_strides), in_of(d->y, d->y_strides), f, d->C1, d->C2, partial, nullptr, nullptr, nullptr);
    if (launch_ok("ssim_tile_fwd") != MM_OK) return MM_ERR_LAUNCH;
    hipLaunchKernelGGL(ssim_fold_kernel, dim3(1), dim3(1024), 0, stream, partial, planes, ntiles, d->C, (float)f.Ho * (float)f.Wo,
                       (d->flags & MM_SSIM_NONNEG) ? 1 : 0, d->ssim, d->cs, d->mean_c, d->mean_all);
    return launch_ok("ssim_fold");
}

int launch_ssim_bwd(const MMSsimDesc* d, const MMSsimGrads* g, hipStream_t stream) {
    const SsimFilter fo = make_filter(d, true, false);
    const SsimFilter fi = make_filter(d, false, true);
    const int planes = d->N * d->C;
    float* adj = (float*)d->workspace;
    const SsimIn X = in_of(d->x, d->x_strides), Y = in_of(d->y, d->y_strides);
    hipLaunchKernelGGL(ssim_tile_kernel<true>, dim3(planes * fo.ntx * fo.nty), dim3(SS_THREADS), tile_lds_bytes(fo, 2), stream,
                       X, Y, fo, d->C1, d->C2, nullptr, g->grad_ssim, g->grad_cs, adj);
    if (launch_ok("ssim_tile_bwd") != MM_OK) return MM_ERR_LAUNCH;
    hipLaunchKernelGGL(ssim_gather_kernel, dim3(planes * fi.ntx * fi.nty), dim3(SS_THREADS), tile_lds_bytes(fi, 1), stream,
                       X, Y, fi, (const float*)adj, g->grad_x, g->grad_y);
    return launch_ok("ssim_gather_bwd");
}

}  // namespace mm
