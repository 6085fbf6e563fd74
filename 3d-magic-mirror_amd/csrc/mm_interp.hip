// mm_interp.hip -- the attribute interpolation block of the reference's generator step for gfx950 (trainer.py:293-342).
//
// Replaces, between render #1 and render #2:
//   mean_delta = mean(|delta_vertices[:, -1]|, 1); bad = mean_delta > 0.4      (a device -> host copy in the reference)
//   rand_a / rand_b: permutations whose slots holding a bad sample are redrawn from the good ones (numpy in the reference)
//   Aa = deep_copy(Ae, rand_a); Ab = deep_copy(Ae, rand_b)                     (nine gathers + clones each)
//   X = a * Aa[X] + (1 - a) * Ab[X]  for vertices, delta_vertices (alpha_shape), textures, bg (alpha_texture), lights (alpha_light)
//
// collapse_resample: one 1024-thread workgroup.  Each wave ballots "good" over 64 samples: the ballot IS a 64-bit word of the good
// mask, kept in LDS with the exclusive prefix of the words' popcounts; the m-th good sample is a binary search over that prefix and
// a select inside one word.  B <= 65535 keeps the mask in 8 KiB of LDS.
// mix_fwd: one launch over all five tensors, cut into chunks of one row each (so the row's two indices and its alpha are wave-uniform,
// scalar loads); a grid of at most MM_MIX_GRID workgroups strides over the chunks.  Rows whose length is a multiple of 4 at 16-byte
// aligned addresses (textures, bg) move as float4, the others (vertices: 3V floats, lights: 9) as floats.
// mix_bwd: a gather per SOURCE row over the inverse index lists (who picked this row as a, then as b), each list ascending in the
// output row: no float atomics, a fixed summation order, bitwise reproducible.  mix_lists builds the lists in the workspace with
// one workgroup (integer counts, a scan, and a stable fill in chunks of 1024 output rows).
#include <hip/hip_runtime.h>

#include "mm_device.h"
#include "mm_stream.h"                                        // block_scan_excl: the workgroup scan the encoders' array scans stand on

#define MM_MIX_BLOCK 256
#define MM_MIX_PER_THREAD 4                                   // float4s (or floats) per thread per chunk
#define MM_MIX_GRID 2048                                      // 256 CUs x 8 workgroups (cdna_hip_programming.md, Guideline 11)
#define MM_RS_BLOCK 1024
#define MM_RS_WORDS (65536 / 64)

namespace mm {

struct MixSeg {
    const float* src;                                         // (B, len) source rows
    float* dst;                                               // (B, len): forward output rows / backward source gradient rows
    const float* g;                                           // backward: (B, len) upstream gradient rows
    const float* alpha;                                       // (B)
    long long len;                                            // floats per row
    int vec;                                                  // 1: float4 path
    int nchunk;                                               // chunks per row
    int chunk0;                                               // first chunk id of this tensor
};

struct MixArgs {
    MixSeg seg[5];
    int nseg, B, total;
    const int* ia; const int* ib;
    const int* offs_a; const int* list_a;                     // backward: inverse lists, (B+1) offsets and (B) output rows each
    const int* offs_b; const int* list_b;
};

__device__ inline float4 lerp4(float a, float om, float4 x, float4 y) {
    MM_FP_EXACT
    return make_float4(a * x.x + om * y.x, a * x.y + om * y.y, a * x.z + om * y.z, a * x.w + om * y.w);
}

__device__ inline float4 axpy4(float4 acc, float w, float4 g) {
    MM_FP_EXACT
    return make_float4(acc.x + w * g.x, acc.y + w * g.y, acc.z + w * g.z, acc.w + w * g.w);
}

__device__ inline int seg_of(const MixArgs& a, int c) {
    int t = 0;
    while (t + 1 < a.nseg && c >= a.seg[t + 1].chunk0) ++t;
    return t;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ inline void mix_row_chunk(const T* __restrict__ src, T* __restrict__ dst, long long n, long long e0, int row, int ja, int jb,
                                     float a, bool valid) {
    MM_FP_EXACT
    const float om = 1.0f - a;
    const T* xa = src + (long long)ja * n;
    const T* xb = src + (long long)jb * n;
    T* o = dst + (long long)row * n;
    T va[MM_MIX_PER_THREAD], vb[MM_MIX_PER_THREAD];
#pragma unroll
    for (int k = 0; k < MM_MIX_PER_THREAD; ++k) {
        const long long e = e0 + k * MM_MIX_BLOCK;
        if (valid && e < n) { va[k] = xa[e]; vb[k] = xb[e]; }
    }
#pragma unroll
    for (int k = 0; k < MM_MIX_PER_THREAD; ++k) {
        const long long e = e0 + k * MM_MIX_BLOCK;
        if (e >= n) continue;
        if constexpr (sizeof(T) == 16) o[e] = valid ? lerp4(a, om, va[k], vb[k]) : make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
        else o[e] = valid ? a * va[k] + om * vb[k] : __builtin_nanf("");
    }
}

__global__ __launch_bounds__(MM_MIX_BLOCK) void mix_fwd_kernel(MixArgs a) {
    for (int c = blockIdx.x; c < a.total; c += gridDim.x) {
        const MixSeg& s = a.seg[seg_of(a, c)];
        const int r = c - s.chunk0;
        const int row = r / s.nchunk, part = r - row * s.nchunk;
        const int ja = a.ia[row], jb = a.ib[row];
        const bool valid = ja >= 0 && ja < a.B && jb >= 0 && jb < a.B;   // otherwise a NaN row, and nothing is read
        const float al = s.alpha[row];
        const long long e0 = (long long)part * (MM_MIX_BLOCK * MM_MIX_PER_THREAD) + threadIdx.x;
        if (s.vec) mix_row_chunk((const float4*)s.src, (float4*)s.dst, s.len >> 2, e0, row, valid ? ja : 0, valid ? jb : 0, al, valid);
        else mix_row_chunk(s.src, s.dst, s.len, e0, row, valid ? ja : 0, valid ? jb : 0, al, valid);
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ inline T tzero();
template <> __device__ inline float tzero<float>() { return 0.0f; }
template <> __device__ inline float4 tzero<float4>() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
__device__ inline float axpy(float acc, float w, float g) { MM_FP_EXACT return acc + w * g; }
__device__ inline float4 axpy(float4 acc, float w, float4 g) { return axpy4(acc, w, g); }

template <typename T>
__device__ inline void mix_bwd_chunk(const T* __restrict__ g, T* __restrict__ dst, long long n, long long e0, int row, const MixArgs& a,
                                     const float* __restrict__ alpha) {
    MM_FP_EXACT
    T acc[MM_MIX_PER_THREAD];
#pragma unroll
    for (int k = 0; k < MM_MIX_PER_THREAD; ++k) acc[k] = tzero<T>();
    const int a0 = a.offs_a[row], a1 = a.offs_a[row + 1];
    for (int q = a0; q < a1; ++q) {                           // rows j with ia[j] == row, ascending: + fl(a[j] * g[j])
        const int j = a.list_a[q];
        const float w = alpha[j];
        const T* gj = g + (long long)j * n;
#pragma unroll
        for (int k = 0; k < MM_MIX_PER_THREAD; ++k) {
            const long long e = e0 + k * MM_MIX_BLOCK;
            if (e < n) acc[k] = axpy(acc[k], w, gj[e]);
        }
    }
    const int b0 = a.offs_b[row], b1 = a.offs_b[row + 1];
    for (int q = b0; q < b1; ++q) {                           // then rows j with ib[j] == row, ascending: + fl(fl(1 - a[j]) * g[j])
        const int j = a.list_b[q];
        const float w = 1.0f - alpha[j];
        const T* gj = g + (long long)j * n;
#pragma unroll
        for (int k = 0; k < MM_MIX_PER_THREAD; ++k) {
            const long long e = e0 + k * MM_MIX_BLOCK;
            if (e < n) acc[k] = axpy(acc[k], w, gj[e]);
        }
    }
    T* o = dst + (long long)row * n;
#pragma unroll
    for (int k = 0; k < MM_MIX_PER_THREAD; ++k) {
        const long long e = e0 + k * MM_MIX_BLOCK;
        if (e < n) o[e] = acc[k];
    }
}

__global__ __launch_bounds__(MM_MIX_BLOCK) void mix_bwd_kernel(MixArgs a) {
    for (int c = blockIdx.x; c < a.total; c += gridDim.x) {
        const MixSeg& s = a.seg[seg_of(a, c)];
        const int r = c - s.chunk0;
        const int row = r / s.nchunk, part = r - row * s.nchunk;
        const long long e0 = (long long)part * (MM_MIX_BLOCK * MM_MIX_PER_THREAD) + threadIdx.x;
        if (s.vec) mix_bwd_chunk((const float4*)s.g, (float4*)s.dst, s.len >> 2, e0, row, a, s.alpha);
        else mix_bwd_chunk(s.g, s.dst, s.len, e0, row, a, s.alpha);
    }
}

// a read of a word that integer atomics of this workgroup have changed: at agent scope, so it is served by L2 (where atomics land)
__device__ inline int ld_l2(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// offs (B+1): exclusive prefix of the counts cur (B) holds on entry; cur is left equal to offs[0..B).  sh: as block_scan_excl wants it
__device__ inline void counts_to_offsets(int B, int* cur, int* offs, int* sh) {
    const int t = threadIdx.x;
    const int per = (B + MM_RS_BLOCK - 1) / MM_RS_BLOCK;
    const int lo = min(B, t * per), hi = min(B, lo + per);
    int sum = 0, total;
    for (int i = lo; i < hi; ++i) sum += ld_l2(&cur[i]);
    int run = block_scan_excl<MM_RS_BLOCK>(sum, t, sh, total);
    for (int i = lo; i < hi; ++i) {
        const int c = ld_l2(&cur[i]);
        offs[i] = run;
        cur[i] = run;
        run += c;
    }
    if (t == MM_RS_BLOCK - 1) offs[B] = run;
}

// the inverse index lists of the backward: for every source row i, the output rows j with ia[j] == i (list_a) and with ib[j] == i
// (list_b), ascending in j; indices outside [0, B) are left out.  One workgroup.
__global__ __launch_bounds__(MM_RS_BLOCK) void mix_lists_kernel(int B, const int* __restrict__ ia, const int* __restrict__ ib, int* offs_a,
                                                                int* list_a, int* cur_a, int* offs_b, int* list_b, int* cur_b) {
    __shared__ int sh[block_scan_words<MM_RS_BLOCK, int>()];
    __shared__ int ka_s[MM_RS_BLOCK], kb_s[MM_RS_BLOCK];
    const int t = threadIdx.x;
    for (int i = t; i < B; i += MM_RS_BLOCK) { cur_a[i] = 0; cur_b[i] = 0; }
    __syncthreads();
    for (int j = t; j < B; j += MM_RS_BLOCK) {
        const int ka = ia[j], kb = ib[j];
        if (ka >= 0 && ka < B) atomicAdd(&cur_a[ka], 1);
        if (kb >= 0 && kb < B) atomicAdd(&cur_b[kb], 1);
    }
    __syncthreads();
    counts_to_offsets(B, cur_a, offs_a, sh);
    counts_to_offsets(B, cur_b, offs_b, sh);
    __syncthreads();
    for (int base = 0; base < B; base += MM_RS_BLOCK) {       // stable fill: rank among the chunk's earlier rows with the same key
        const int j = base + t;
        int ka = j < B ? ia[j] : -1, kb = j < B ? ib[j] : -1;
        if (ka < 0 || ka >= B) ka = -1;
        if (kb < 0 || kb >= B) kb = -1;
        ka_s[t] = ka; kb_s[t] = kb;
        __syncthreads();
        int ra = 0, rb = 0;
        if (j < B)                                            // rows past B hold no key: nothing to rank, nobody ranks against them
            for (int u = 0; u < t; ++u) { ra += ka_s[u] == ka; rb += kb_s[u] == kb; }
        const int pa = ka >= 0 ? ld_l2(&cur_a[ka]) + ra : 0, pb = kb >= 0 ? ld_l2(&cur_b[kb]) + rb : 0;
        __syncthreads();                                      // every cursor read before any is advanced
        if (ka >= 0) { list_a[pa] = j; atomicMax(&cur_a[ka], pa + 1); }
        if (kb >= 0) { list_b[pb] = j; atomicMax(&cur_b[kb], pb + 1); }
        __syncthreads();
    }
}

// ---- collapse resampling ---------------------------------------------------------------------------------------------------------
// bad[b] = ((|x| + |y|) + |z|) / 3 > thr over delta_vertices[b, V-1, :]; a NaN mean is not bad.  Every slot s of idx_a (idx_b) holding a
// bad sample gets good[min(floor(fl(u[0,s] * n_good)), n_good - 1)] (u[1,s] for idx_b), good = the samples that are not bad, ascending.
// No good sample: the indices stay, n_bad = B.
__device__ inline int select_bit(uint64_t w, int r) {        // position of the r-th (0-based) set bit of w; r < popcount(w)
    int pos = 0;
    for (int width = 32; width >= 1; width >>= 1) {
        const int c = __popcll(w & ((1ull << width) - 1));
        if (r >= c) { r -= c; w >>= width; pos += width; }
    }
    return pos;
}

__global__ __launch_bounds__(MM_RS_BLOCK) void collapse_resample_kernel(int B, int V, const float* __restrict__ dv, int* idx_a, int* idx_b,
                                                                        const float* __restrict__ u, float thr, int* n_bad) {
    MM_FP_EXACT
    __shared__ uint64_t good_w[MM_RS_WORDS];
    __shared__ int pre[MM_RS_WORDS + 1];
    __shared__ int sh[block_scan_words<MM_RS_BLOCK, int>()];
    const int t = threadIdx.x, lane = t & (MM_WAVE - 1);
    const int nwords = (B + MM_WAVE - 1) / MM_WAVE;
    for (int base = 0; base < nwords * MM_WAVE; base += MM_RS_BLOCK) {
        const int b = base + t;
        bool good = false;
        if (b < B) {
            const float* p = dv + ((long long)b * V + (V - 1)) * 3;
            const float m = ((fabsf(p[0]) + fabsf(p[1])) + fabsf(p[2])) / 3.0f;
            good = !(m > thr);
        }
        const uint64_t w = __ballot(good);
        if (lane == 0 && b < nwords * MM_WAVE) good_w[b >> 6] = w;
    }
    __syncthreads();
    const int cnt = t < nwords ? __popcll(good_w[t]) : 0;      // nwords <= 1024: one word per thread
    int total;
    const int excl = block_scan_excl<MM_RS_BLOCK>(cnt, t, sh, total);
    if (t < nwords) pre[t] = excl;
    if (t == MM_RS_BLOCK - 1) pre[nwords] = total;
    __syncthreads();
    const int n_good = pre[nwords];
    if (t == 0) *n_bad = B - n_good;
    if (n_good == 0) return;
    for (int s = t; s < B; s += MM_RS_BLOCK) {
        for (int which = 0; which < 2; ++which) {
            int* idx = which ? idx_b : idx_a;
            const int k = idx[s];
            if (k < 0 || k >= B || ((good_w[k >> 6] >> (k & 63)) & 1)) continue;
            const float f = u[which * B + s] * (float)n_good;
            const int m = f >= 1.0f ? min((int)f, n_good - 1) : 0;   // also catches a NaN or negative uniform
            int lo = 0, hi = nwords - 1;                        // the last word whose prefix is <= m
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pre[mid] <= m) lo = mid; else hi = mid - 1;
            }
            idx[s] = lo * MM_WAVE + select_bit(good_w[lo], m - pre[lo]);
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct MixLists { int *offs_a, *list_a, *cur_a, *offs_b, *list_b, *cur_b; size_t bytes; };

static MixLists carve_lists(void* base, int B) {
    MixLists l;
    char* p = (char*)base;
    size_t o = 0;
    int** slots[6] = {&l.offs_a, &l.list_a, &l.cur_a, &l.offs_b, &l.list_b, &l.cur_b};
    for (int i = 0; i < 6; ++i) {
        *slots[i] = (int*)(p + o);
        o += align256((size_t)(B + 1) * 4);
    }
    l.bytes = o;
    return l;
}

size_t interp_workspace_bytes(int B) { return carve_lists(nullptr, B).bytes; }

static void add_seg(MixArgs& a, const float* src, float* dst, const float* g, const float* alpha, long long len) {
    MixSeg& s = a.seg[a.nseg++];
    s.src = src; s.dst = dst; s.g = g; s.alpha = alpha; s.len = len;
    const uintptr_t addr = (uintptr_t)src | (uintptr_t)dst | (uintptr_t)g;
    s.vec = (len % 4 == 0) && (addr % 16 == 0);
    const long long per = (long long)MM_MIX_BLOCK * MM_MIX_PER_THREAD * (s.vec ? 4 : 1);
    s.nchunk = (int)((len + per - 1) / per);
    s.chunk0 = a.total;
    a.total += a.B * s.nchunk;
}

static long long row_len(const MMInterpDesc* d, int t) {
    switch (t) {
        case 0: case 1: return 3LL * d->V;
        case 2: return 3LL * d->Ht * d->Wt;
        case 3: return 3LL * d->H * d->W;
        default: return 9;
    }
}

static dim3 mix_grid(int total) { return dim3((unsigned)(total < MM_MIX_GRID ? total : MM_MIX_GRID)); }

int launch_mix_fwd(const MMInterpDesc* d, hipStream_t s) {
    MixArgs a = {};
    a.B = d->B; a.ia = d->idx_a; a.ib = d->idx_b;
    const float* src[5] = {d->vertices, d->delta_vertices, d->textures, d->bg, d->lights};
    float* out[5] = {d->out_vertices, d->out_delta_vertices, d->out_textures, d->out_bg, d->out_lights};
    const float* al[5] = {d->alpha_shape, d->alpha_shape, d->alpha_texture, d->alpha_texture, d->alpha_light};
    for (int t = 0; t < 5; ++t)
        if (src[t]) add_seg(a, src[t], out[t], nullptr, al[t], row_len(d, t));
    hipLaunchKernelGGL(mix_fwd_kernel, mix_grid(a.total), dim3(MM_MIX_BLOCK), 0, s, a);
    return launch_ok("attribute_mix_fwd");
}

int launch_mix_bwd(const MMInterpDesc* d, const MMInterpGrads* g, hipStream_t s) {
    MixArgs a = {};
    a.B = d->B; a.ia = d->idx_a; a.ib = d->idx_b;
    const float* up[5] = {g->grad_out_vertices, g->grad_out_delta_vertices, g->grad_out_textures, g->grad_out_bg, g->grad_out_lights};
    float* gs[5] = {g->grad_vertices, g->grad_delta_vertices, g->grad_textures, g->grad_bg, g->grad_lights};
    const float* al[5] = {d->alpha_shape, d->alpha_shape, d->alpha_texture, d->alpha_texture, d->alpha_light};
    for (int t = 0; t < 5; ++t)
        if (up[t] && gs[t]) add_seg(a, nullptr, gs[t], up[t], al[t], row_len(d, t));
    if (a.nseg == 0) return MM_OK;                            // no upstream gradient at all: nothing to launch
    const MixLists l = carve_lists(d->workspace, d->B);
    hipLaunchKernelGGL(mix_lists_kernel, dim3(1), dim3(MM_RS_BLOCK), 0, s, d->B, d->idx_a, d->idx_b, l.offs_a, l.list_a, l.cur_a, l.offs_b,
                       l.list_b, l.cur_b);
    a.offs_a = l.offs_a; a.list_a = l.list_a; a.offs_b = l.offs_b; a.list_b = l.list_b;
    hipLaunchKernelGGL(mix_bwd_kernel, mix_grid(a.total), dim3(MM_MIX_BLOCK), 0, s, a);
    return launch_ok("attribute_mix_bwd");
}

int launch_collapse_resample(int B, int V, const float* dv, int* idx_a, int* idx_b, const float* u, float thr, int* n_bad, hipStream_t s) {
    hipLaunchKernelGGL(collapse_resample_kernel, dim3(1), dim3(MM_RS_BLOCK), 0, s, B, V, dv, idx_a, idx_b, u, thr, n_bad);
    return launch_ok("collapse_resample");
}

}  // namespace mm
