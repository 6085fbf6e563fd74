// mm_fid.hip -- what surrounds the Inception network in an FID evaluation, for gfx950: the network's input batch from 8-bit device frames, and
// the float64 mean and covariance of its features (fid_score.py:71-255, inception.py:129-163).  The network itself stays stock PyTorch.
//
// fid_input_kernel   (n,H,W,3) bytes -> (n,3,Ho,Wo) fp32 planes: v / 255, torch's bilinear resize with align_corners=False, 2 x - 1.  The two
//                    axes arrive lowered as rows {i0, i1, w0, w1} (frames.resize_taps: two taps; a dropped tap has weight 0 and i1 clamped).
//                    Arithmetic, every step rounded in fp32, nothing contracted (the file is compiled EXACT):
//                      t(b)  = fl(float(b) / 255.0f)                               IEEE division (a 256-entry table in LDS, built by it)
//                      h(r)  = fl(fl(w0x * t(r, i0x)) + fl(w1x * t(r, i1x)))        horizontal, on source rows r = i0y, i1y
//                      v     = fl(fl(w0y * h(i0y)) + fl(w1y * h(i1y)))              vertical
//                      out   = fl(fl(2 * v) - 1)                                   with normalize; v otherwise
//                    A workgroup owns MM_FID_ROWS output rows of one frame, all three planes: it stages the two source rows of each output
//                    row in LDS as bytes, and its lanes issue 16-byte stores on the FLAT output (a plane's rows are not multiples of four
//                    floats: 299 * 299 is odd) -- the floats before the first and after the last aligned chunk of its range go one by one.
//                    One launch, no workspace, no atomics; every output float is written by one lane.
//
// fid statistics     mean and covariance of N feature rows (N,D) fp32, as np.mean(act, 0) and np.cov(act, rowvar=False) of their float64 copy,
//                    without forming that copy.  Four launches, no atomics, every order fixed (bitwise reproducible):
//   fid_colsum_kernel  column sums in float64 of chunks of MM_FID_SUM_ROWS rows, rows ascending, one lane per column -> workspace
//   fid_mean_kernel    mu[c] = (chunks added ascending) / N
//   fid_gram_kernel    the centred Gram matrix Xc^T Xc on v_mfma_f64_16x16x4_f64.  A workgroup owns a 64 x 64 macro-tile (I, J), I <= J only, and
//                      a split of MM_FID_SPLIT rows; it stages 16 rows of both column blocks in LDS as f64: loaded as fp32 (a stage ahead, into
//                      registers, so that the loads are in flight while the stage before is multiplied), widened and centred by mu in f64
//                      (np.cov's X -= avg); rows >= N and columns >= D enter as zeros and are never loaded.  Each of its four waves
//                      holds a 32 x 32 block as 2 x 2 accumulators and steps four rows per instruction, rows ascending.  Fragment maps of the
//                      f64 form: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], C/D col = l & 15, row = (l >> 4) + 4 * reg.
//                      The (split, tile) partial goes to the workspace.
//   fid_cov_kernel     adds a tile's splits ascending, divides ONCE by N - 1 and writes (i, j) and (j, i) from the same value (only i <= j is
//                      read): sigma is exactly symmetric.
#include <hip/hip_runtime.h>

#include "mm_device.h"

#define MM_FID_BLOCK 256
#define MM_FID_ROWS 8                                         // output rows per workgroup of fid_input_kernel
#define MM_FID_TILE 64                                        // macro-tile of the Gram matrix
#define MM_FID_KC 16                                          // rows per LDS stage (a multiple of 4)
#define MM_FID_PITCH 80                                       // doubles per staged row: 64 + 16, so that a wave's four rows spread over all banks

namespace mm {

// ---- Inception inputs -------------------------------------------------------------------------------------------------------------
struct FidInputArgs {
    const unsigned char* frames;
    const int4* xrows; const int4* yrows;                     // {i0, i1, w0 bits, w1 bits}
    float* out;
    int H, W, Ho, Wo, normalize, bands, vec;
};

// output element e of the band's range in plane c: e = j * Wo + x, j the row inside the band
__device__ inline float fid_input_value(const FidInputArgs& a, const unsigned char* s_rows, const float* s_lut, const float2* s_wy, int c, int j, int x) {
    MM_FP_EXACT
    const int4 xr = a.xrows[x];
    const float w0 = __int_as_float(xr.z), w1 = __int_as_float(xr.w);
    const unsigned char* r0 = s_rows + (size_t)(2 * j) * a.W * 3;
    const unsigned char* r1 = r0 + (size_t)a.W * 3;
    const float h0 = w0 * s_lut[r0[xr.x * 3 + c]] + w1 * s_lut[r0[xr.y * 3 + c]];
    const float h1 = w0 * s_lut[r1[xr.x * 3 + c]] + w1 * s_lut[r1[xr.y * 3 + c]];
    const float2 wy = s_wy[j];
    const float v = wy.x * h0 + wy.y * h1;
    return a.normalize ? 2.0f * v - 1.0f : v;
}

__global__ __launch_bounds__(MM_FID_BLOCK) void fid_input_kernel(FidInputArgs a) {
    extern __shared__ unsigned char s_dyn[];                  // 256 floats, MM_FID_ROWS float2, then 2 * MM_FID_ROWS rows of W * 3 bytes
    float* s_lut = (float*)s_dyn;
    float2* s_wy = (float2*)(s_lut + 256);
    unsigned char* s_rows = (unsigned char*)(s_wy + MM_FID_ROWS);
    const int tid = threadIdx.x;
    const int f = blockIdx.x / a.bands, band = blockIdx.x - f * a.bands;
    const int row0 = band * MM_FID_ROWS;
    const int rows = min(MM_FID_ROWS, a.Ho - row0);
    const int rb = a.W * 3;
    {
        MM_FP_EXACT
        s_lut[tid] = (float)tid / 255.0f;
    }
    const unsigned char* frame = a.frames + (size_t)f * a.H * rb;
    for (int s = 0; s < 2 * rows; ++s) {
        const int4 yr = a.yrows[row0 + (s >> 1)];
        if (tid == 0 && !(s & 1)) s_wy[s >> 1] = make_float2(__int_as_float(yr.z), __int_as_float(yr.w));
        const unsigned char* src = frame + (size_t)((s & 1) ? yr.y : yr.x) * rb;
        for (int i = tid; i < rb; i += MM_FID_BLOCK) s_rows[(size_t)s * rb + i] = src[i];
    }
    __syncthreads();
    const long long plane = (long long)a.Ho * a.Wo;
    const int len = rows * a.Wo;
    for (int c = 0; c < 3; ++c) {
        const long long base = ((long long)f * 3 + c) * plane + (long long)row0 * a.Wo;
        float* o = a.out + base;
        const int head = a.vec ? min(len, (int)((4 - (base & 3)) & 3)) : len;
        const int nvec = (len - head) >> 2;
        const int tail = len - head - 4 * nvec;
        for (int q = tid; q < nvec; q += MM_FID_BLOCK) {
            const int e = head + 4 * q;
            int j = e / a.Wo, x = e - j * a.Wo;
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = fid_input_value(a, s_rows, s_lut, s_wy, c, j, x);
                if (++x == a.Wo) { x = 0; ++j; }
            }
            *(float4*)(o + e) = make_float4(v[0], v[1], v[2], v[3]);
        }
        for (int t = tid; t < head + tail; t += MM_FID_BLOCK) {
            const int e = t < head ? t : head + 4 * nvec + (t - head);
            const int j = e / a.Wo;
            o[e] = fid_input_value(a, s_rows, s_lut, s_wy, c, j, e - j * a.Wo);
        }
    }
}

long long fid_input_lds_bytes(const MMFidInputDesc* d) {
    return 256 * (long long)sizeof(float) + MM_FID_ROWS * (long long)sizeof(float2) + 2LL * MM_FID_ROWS * d->W * 3;
}

int launch_fid_input(const MMFidInputDesc* d, hipStream_t s) {
    FidInputArgs a;
    a.frames = d->frames; a.xrows = (const int4*)d->params; a.yrows = a.xrows + d->Wo; a.out = d->out;
    a.H = d->H; a.W = d->W; a.Ho = d->Ho; a.Wo = d->Wo; a.normalize = d->normalize != 0;
    a.bands = (d->Ho + MM_FID_ROWS - 1) / MM_FID_ROWS;
    a.vec = ((uintptr_t)d->out & 15) == 0;
    hipLaunchKernelGGL(fid_input_kernel, dim3((unsigned)((long long)d->n * a.bands)), dim3(MM_FID_BLOCK), (size_t)fid_input_lds_bytes(d), s, a);
    return launch_ok("fid_input");
}

// ---- statistics ---------------------------------------------------------------------------------------------------------------------
typedef double fid_d4 __attribute__((ext_vector_type(4)));

struct FidStatsLayout { size_t colsum, gram, bytes; int chunks, splits, T; long long tiles; };

FidStatsLayout fid_stats_layout(const MMFidStatsDesc* d) {
    FidStatsLayout l;
    l.chunks = (d->N + MM_FID_SUM_ROWS - 1) / MM_FID_SUM_ROWS;
    l.splits = (d->N + MM_FID_SPLIT - 1) / MM_FID_SPLIT;
    l.T = (d->D + MM_FID_TILE - 1) / MM_FID_TILE;
    l.tiles = (long long)l.T * (l.T + 1) / 2;
    l.colsum = 0;
    l.gram = align256((size_t)l.chunks * d->D * sizeof(double));
    l.bytes = l.gram + align256((size_t)l.splits * l.tiles * MM_FID_TILE * MM_FID_TILE * sizeof(double));
    return l;
}

size_t fid_stats_workspace_bytes(const MMFidStatsDesc* d) { return fid_stats_layout(d).bytes; }
long long fid_stats_tiles(const MMFidStatsDesc* d) { return fid_stats_layout(d).tiles; }

__global__ __launch_bounds__(MM_FID_BLOCK) void fid_colsum_kernel(const float* __restrict__ x, int N, int D, double* __restrict__ part) {
    const int c = blockIdx.x * MM_FID_BLOCK + threadIdx.x;
    if (c >= D) return;
    const int n0 = blockIdx.y * MM_FID_SUM_ROWS, n1 = min(N, n0 + MM_FID_SUM_ROWS);
    double s = 0.0;
    for (int n = n0; n < n1; ++n) s += (double)x[(size_t)n * D + c];
    part[(size_t)blockIdx.y * D + c] = s;
}

__global__ __launch_bounds__(MM_FID_BLOCK) void fid_mean_kernel(const double* __restrict__ part, int chunks, int N, int D, double* __restrict__ mu) {
    const int c = blockIdx.x * MM_FID_BLOCK + threadIdx.x;
    if (c >= D) return;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += part[(size_t)k * D + c];
    mu[c] = s / (double)N;
}

// upper-triangle tile t of T block rows, row-major: (I, J) with I <= J
__device__ inline void fid_tile_of(long long t, int T, int& I, int& J) {
    I = 0;
    while (t >= T - I) { t -= T - I; ++I; }
    J = I + (int)t;
}

__global__ __launch_bounds__(MM_FID_BLOCK) void fid_gram_kernel(const float* __restrict__ x, const double* __restrict__ mu, int N, int D, int T,
                                                                 long long tiles, double* __restrict__ gram) {
    __shared__ double sA[MM_FID_KC][MM_FID_PITCH], sB[MM_FID_KC][MM_FID_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = MM_WAVE_UNIFORM(tid >> 6);
    int I, J;
    fid_tile_of(blockIdx.x, T, I, J);
    const int split = blockIdx.y;
    const int n_begin = split * MM_FID_SPLIT, n_end = min(N, n_begin + MM_FID_SPLIT);
    // staging: this thread's column of both blocks, rows (tid >> 6) + 4 r of the stage
    const int sc = tid & 63, sr = tid >> 6;
    const int ca = I * MM_FID_TILE + sc, cb = J * MM_FID_TILE + sc;
    const double ma = ca < D ? mu[ca] : 0.0, mb = cb < D ? mu[cb] : 0.0;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    fid_d4 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = (fid_d4){0.0, 0.0, 0.0, 0.0};
    // the stage's fp32 values wait in registers: the loads of stage s + 1 are in flight while stage s is multiplied
    float ra[MM_FID_KC / 4], rb[MM_FID_KC / 4];
    auto fetch = [&](int n0) {
#pragma unroll
        for (int r = 0; r < MM_FID_KC / 4; ++r) {
            const int n = n0 + sr + 4 * r;
            ra[r] = (n < n_end && ca < D) ? x[(size_t)n * D + ca] : 0.0f;
            rb[r] = (n < n_end && cb < D) ? x[(size_t)n * D + cb] : 0.0f;
        }
    };
    fetch(n_begin);
    for (int n0 = n_begin; n0 < n_end; n0 += MM_FID_KC) {
#pragma unroll
        for (int r = 0; r < MM_FID_KC / 4; ++r) {
            const int k = sr + 4 * r;
            const bool in = n0 + k < n_end;                       // a row beyond N is zero, not minus mu
            sA[k][sc] = (in && ca < D) ? (double)ra[r] - ma : 0.0;
            sB[k][sc] = (in && cb < D) ? (double)rb[r] - mb : 0.0;
        }
        __syncthreads();
        if (n0 + MM_FID_KC < n_end) fetch(n0 + MM_FID_KC);
#pragma unroll
        for (int k0 = 0; k0 < MM_FID_KC; k0 += 4) {
            const int k = k0 + (lane >> 4), m = lane & 15;
            const double a0 = sA[k][wi + m], a1 = sA[k][wi + 16 + m];
            const double b0 = sB[k][wj + m], b1 = sB[k][wj + 16 + m];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    double* g = gram + ((size_t)split * tiles + blockIdx.x) * (MM_FID_TILE * MM_FID_TILE);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int i = wi + 16 * p + (lane >> 4) + 4 * reg, j = wj + 16 * q + (lane & 15);
                g[i * MM_FID_TILE + j] = acc[p][q][reg];
            }
}

__global__ __launch_bounds__(MM_FID_BLOCK) void fid_cov_kernel(const double* __restrict__ gram, int splits, long long tiles, int N, int D, int T,
                                                                double* __restrict__ sigma) {
    int I, J;
    fid_tile_of(blockIdx.x, T, I, J);
    const double* g = gram + (size_t)blockIdx.x * (MM_FID_TILE * MM_FID_TILE);
    const double denom = (double)(N - 1);
    for (int e = threadIdx.x; e < MM_FID_TILE * MM_FID_TILE; e += MM_FID_BLOCK) {
        const int i = I * MM_FID_TILE + (e >> 6), j = J * MM_FID_TILE + (e & 63);
        if (i >= D || j >= D || i > j) continue;
        double s = 0.0;
        for (int k = 0; k < splits; ++k) s += g[(size_t)k * tiles * (MM_FID_TILE * MM_FID_TILE) + e];
        const double v = s / denom;
        sigma[(size_t)i * D + j] = v;
        sigma[(size_t)j * D + i] = v;
    }
}

int launch_fid_stats(const MMFidStatsDesc* d, hipStream_t s) {
    const FidStatsLayout l = fid_stats_layout(d);
    double* part = (double*)((char*)d->workspace + l.colsum);
    double* gram = (double*)((char*)d->workspace + l.gram);
    const unsigned cols = (unsigned)((d->D + MM_FID_BLOCK - 1) / MM_FID_BLOCK);
    hipLaunchKernelGGL(fid_colsum_kernel, dim3(cols, (unsigned)l.chunks), dim3(MM_FID_BLOCK), 0, s, d->x, d->N, d->D, part);
    int st = launch_ok("fid_colsum");
    if (st != MM_OK) return st;
    hipLaunchKernelGGL(fid_mean_kernel, dim3(cols), dim3(MM_FID_BLOCK), 0, s, part, l.chunks, d->N, d->D, d->mu);
    st = launch_ok("fid_mean");
    if (st != MM_OK) return st;
    hipLaunchKernelGGL(fid_gram_kernel, dim3((unsigned)l.tiles, (unsigned)l.splits), dim3(MM_FID_BLOCK), 0, s, d->x, d->mu, d->N, d->D, l.T, l.tiles, gram);
    st = launch_ok("fid_gram");
    if (st != MM_OK) return st;
    hipLaunchKernelGGL(fid_cov_kernel, dim3((unsigned)l.tiles), dim3(MM_FID_BLOCK), 0, s, gram, l.splits, l.tiles, d->N, d->D, l.T, d->sigma);
    return launch_ok("fid_cov");
}

}  // namespace mm
