// mm_encfeat.hip -- template-anchored features of the shape and camera encoders for gfx950.
//
// Replaces the block the reference runs between an encoder's backbone and its heads (network/model_res.py):
//   ShapeEncoder  (:318-327)  local = grid_sample(x, template[..., :2], bilinear, align_corners=True, zeros)     (B,C,V,1)
//                             glob  = MMPool((1,1))(x).repeat(1, 1, V, 1)
//                             neighbor_diff = torch.mm(local.view(-1, V), lpl)     -- a (V,V) DENSE uniform Laplacian
//                             cat((local, glob, neighbor_diff, xyz), 1).squeeze(3)                            (B,3C+3,V)
//   CameraEncoder (:198-200)  cat((MMPool((2,2))(x), MMPool((2,2))(grid_sample(x, uv, align_corners=False))), 1)  (B,2C,2,2)
// with MMPool = sigmoid(p) * adaptive_max + (1 - sigmoid(p)) * adaptive_avg (:23-41).
//
// One 256-thread workgroup per (b, c) plane in each direction.  The forward stages the plane in LDS (when it has at most
// MM_ENC_PLANE_LDS pixels; larger planes are read through the caller's strides), reduces it, samples every vertex from it into
// LDS and writes the output rows along V (coalesced); the shape forward then gathers each column's few lpl non-zeros from the
// sampled row in LDS -- the sparse product the dense (V,V) matrix stands for.  The camera forward never materialises the
// sampled row: it is reduced into its two vertex bins as it is formed.
// The backward is a gather with no float atomics: per plane the gradient of the sampled row goes to LDS (the shape op adds the
// lpl-row gather of d neighbor), and every pixel sums the (vertex, weight) list of the bilinear taps that land on it.  That list
// is the same for every image (one template); pix_list (count) / pix_scan / pix_list (fill) build it per call, ordered by vertex,
// with a wave ballot per pixel.  The p gradients are summed per plane, then over planes in index order (dp_reduce).
#include <hip/hip_runtime.h>

#include "mm_device.h"

#define MM_ENC_BLOCK 256
#define MM_ENC_WAVES (MM_ENC_BLOCK / MM_WAVE)
#define MM_ENC_PLANE_LDS 1024   // planes of at most this many pixels are staged in LDS by the forward

namespace mm {

struct Bf16 { uint16_t u; };

__device__ inline float ld_elem(const float* p) { return *p; }
__device__ inline float ld_elem(const _Float16* p) { return (float)*p; }
__device__ inline float ld_elem(const Bf16* p) { return __uint_as_float((unsigned)p->u << 16); }
__device__ inline void st_elem(float* p, float v) { *p = v; }
__device__ inline void st_elem(_Float16* p, float v) { *p = (_Float16)v; }                 // round to nearest even
__device__ inline void st_elem(Bf16* p, float v) {                                            // round to nearest even; NaN stays NaN
    const unsigned u = __float_as_uint(v);
    p->u = (v != v) ? (uint16_t)0x7FC0 : (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

struct EncArgs {
    int B, C, H, W, V, hw;
    const void* x;
    long long s0, s1, s2, s3;
    const float* tmpl;                        // (V,3)
    bool align;                               // grid_sample align_corners
    int col_k, row_k;
    const int* col_idx; const float* col_val; // (col_k,V)
    const int* row_idx; const float* row_val; // (row_k,V)
    const float* p0; const float* p1;         // shape: p; camera: p_map, p_local
    float* out;
    const float* g;                           // grad_out
    void* gx;                                 // grad_x (B,C,H,W) dense in x's dtype, or null
    const int* pix_off;                       // (hw+1)
    const int* pix_v; const float* pix_w;     // (4V)
    float* part;                              // per-plane partial sums of the p gradients: (nparts, B*C)
    int group;                                // lanes per pixel in the backward's gather (power of two <= 64)
};

// ---- bilinear taps of one template vertex, ATen's grid_sampler_2d (bilinear, zeros padding) ---------------------------------
struct Taps { int idx[4]; float w[4]; };     // pixel h*W + w of the nw, ne, sw, se taps (-1 = outside: reads 0)

__device__ inline Taps vertex_taps(const float* tmpl, int v, int H, int W, bool align) {
    MM_FP_EXACT
    const float gx = tmpl[3 * v], gy = tmpl[3 * v + 1];
    const float ix = align ? ((gx + 1.f) / 2.f) * (float)(W - 1) : ((gx + 1.f) * (float)W - 1.f) / 2.f;
    const float iy = align ? ((gy + 1.f) / 2.f) * (float)(H - 1) : ((gy + 1.f) * (float)H - 1.f) / 2.f;
    Taps t;
#pragma unroll
    for (int k = 0; k < 4; ++k) { t.idx[k] = -1; t.w[k] = 0.f; }
    if (!(fabsf(ix) < 1e9f && fabsf(iy) < 1e9f)) return t;          // NaN / inf / far outside: every tap outside
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    t.w[0] = (fx + 1.f - ix) * (fy + 1.f - iy);
    t.w[1] = (ix - fx) * (fy + 1.f - iy);
    t.w[2] = (fx + 1.f - ix) * (iy - fy);
    t.w[3] = (ix - fx) * (iy - fy);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
        t.idx[k] = (xx >= 0 && xx < W && yy >= 0 && yy < H) ? yy * W + xx : -1;
    }
    return t;
}

// ---- reductions with a fixed order ----------------------------------------------------------------------------------------
// (value, index) of a maximum; ties and NaN as ATen's adaptive_max_pool2d: a NaN wins, and of equal values the FIRST in index order
struct MaxArg { float v; int i; };
__device__ inline MaxArg max_first(MaxArg a, MaxArg b) {
    const bool an = a.v != a.v, bn = b.v != b.v;
    const bool take = (bn && !an) || (!an && b.v > a.v) || ((b.v == a.v || (an && bn)) && b.i < a.i);
    return take ? b : a;
}
__device__ inline MaxArg max_init() { return MaxArg{-INFINITY, 0x7fffffff}; }

// NS sums and NM maxima over the workgroup.  Butterflies inside each wave (both partners add the same two numbers, so every lane
// holds the same bits), then the four waves' results in wave order.  Every thread returns the totals.  red: LDS of
// MM_ENC_WAVES * (NS + 2 NM) words; the closing barrier makes red reusable and everything written before the call visible.
template <int NS, int NM>
__device__ inline void block_reduce(float (&s)[NS], MaxArg (&m)[NM], float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] += __shfl_xor(s[k], o);
#pragma unroll
        for (int k = 0; k < NM; ++k) m[k] = max_first(m[k], MaxArg{__shfl_xor(m[k].v, o), __shfl_xor(m[k].i, o)});
    }
    constexpr int R = NS + 2 * NM;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) red[wave * R + k] = s[k];
#pragma unroll
        for (int k = 0; k < NM; ++k) { red[wave * R + NS + 2 * k] = m[k].v; red[wave * R + NS + 2 * k + 1] = __int_as_float(m[k].i); }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        float t = red[k];
        for (int w = 1; w < MM_ENC_WAVES; ++w) t += red[w * R + k];
        s[k] = t;
    }
#pragma unroll
    for (int k = 0; k < NM; ++k) {
        MaxArg t{red[NS + 2 * k], __float_as_int(red[NS + 2 * k + 1])};
        for (int w = 1; w < MM_ENC_WAVES; ++w) t = max_first(t, MaxArg{red[w * R + NS + 2 * k], __float_as_int(red[w * R + NS + 2 * k + 1])});
        m[k] = t;
    }
    __syncthreads();
}

__device__ inline float sigmoidf_(float p) { return 1.f / (1.f + expf(-p)); }

// adaptive-pool bin i of k over n: [floor(i n / k), ceil((i + 1) n / k))
__device__ inline int bin_lo(int i, int n, int k) { return (int)(((long long)i * n) / k); }
__device__ inline int bin_hi(int i, int n, int k) { return (int)(((long long)(i + 1) * n + k - 1) / k); }

template <typename T>
__device__ inline float ld_px(const EncArgs& a, const T* xp, int i) {
    const int y = i / a.W, xx = i - y * a.W;
    return ld_elem(xp + y * a.s2 + xx * a.s3);
}

// the sampled value of vertex v from the plane (staged in LDS, or through the caller's strides)
template <typename T>
__device__ inline float sample_vertex(const EncArgs& a, const T* xp, const float* plane, int v) {
    MM_FP_EXACT
    const Taps t = vertex_taps(a.tmpl, v, a.H, a.W, a.align);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (t.idx[k] >= 0) s += (plane ? plane[t.idx[k]] : ld_px(a, xp, t.idx[k])) * t.w[k];
    return s;
}

// ---- shape features ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(MM_ENC_BLOCK) void shape_fwd_kernel(EncArgs a) {
    MM_FP_EXACT
    extern __shared__ float lds[];                                   // [V] sampled row, then the staged plane
    __shared__ float red[MM_ENC_WAVES * 4];
    const int bc = blockIdx.x, b = bc / a.C, c = bc - b * a.C, tid = threadIdx.x;
    const T* xp = (const T*)a.x + b * a.s0 + c * a.s1;
    float* plane = a.hw <= MM_ENC_PLANE_LDS ? lds + a.V : nullptr;
    float s[1] = {0.f};
    MaxArg m[1] = {max_init()};
    for (int i = tid; i < a.hw; i += MM_ENC_BLOCK) {
        const float v = ld_px(a, xp, i);
        if (plane) plane[i] = v;
        s[0] += v;
        m[0] = max_first(m[0], MaxArg{v, i});
    }
    block_reduce<1, 1>(s, m, red);
    const float w = sigmoidf_(a.p0[0]);
    const float glob = m[0].v * w + (s[0] / (float)a.hw) * (1.f - w);
    const size_t V = a.V, rows = (size_t)3 * a.C + 3;
    float* o = a.out + (size_t)b * rows * V;
    for (int v = tid; v < a.V; v += MM_ENC_BLOCK) {
        const float l = sample_vertex(a, xp, plane, v);
        lds[v] = l;
        o[(size_t)c * V + v] = l;
        o[((size_t)a.C + c) * V + v] = glob;
    }
    if (c == 0)
        for (int i = tid; i < 3 * a.V; i += MM_ENC_BLOCK) {
            const int j = i / a.V, v = i - j * a.V;
            o[((size_t)3 * a.C + j) * V + v] = a.tmpl[3 * v + j];
        }
    __syncthreads();
    for (int u = tid; u < a.V; u += MM_ENC_BLOCK) {
        float n = 0.f;
        for (int k = 0; k < a.col_k; ++k) {
            const int v = a.col_idx[(size_t)k * V + u];
            if (v >= 0) n += lds[v] * a.col_val[(size_t)k * V + u];
        }
        o[((size_t)2 * a.C + c) * V + u] = n;
    }
}

// d x of one plane: every pixel sums the taps that land on it (a.group lanes per pixel, fixed butterfly), plus `extra(p)`; every
// pixel is written.  dl: the gradient of the sampled row, in LDS.
template <typename T, typename Extra>
__device__ inline void gather_pixels(const EncArgs& a, int bc, const float* dl, Extra extra) {
    MM_FP_EXACT
    const int G = a.group, lig = threadIdx.x & (G - 1), ngroups = MM_ENC_BLOCK / G;
    T* gx = (T*)a.gx + (size_t)bc * a.hw;
    for (int p = threadIdx.x / G; p < a.hw; p += ngroups) {        // uniform within a group: its lanes stay together
        float acc = 0.f;
        for (int e = a.pix_off[p] + lig; e < a.pix_off[p + 1]; e += G) acc += a.pix_w[e] * dl[a.pix_v[e]];
        for (int o = G >> 1; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
        if (lig == 0) st_elem(gx + p, extra(p, acc));
    }
}

template <typename T>
__global__ __launch_bounds__(MM_ENC_BLOCK) void shape_bwd_kernel(EncArgs a) {
    MM_FP_EXACT
    extern __shared__ float lds[];                                   // [V] d local
    __shared__ float red[MM_ENC_WAVES * 4];
    const int bc = blockIdx.x, b = bc / a.C, c = bc - b * a.C, tid = threadIdx.x;
    const T* xp = (const T*)a.x + b * a.s0 + c * a.s1;
    const size_t V = a.V, rows = (size_t)3 * a.C + 3;
    const float* gL = a.g + (size_t)b * rows * V + (size_t)c * V;
    const float* gG = gL + (size_t)a.C * V;
    const float* gN = gL + (size_t)2 * a.C * V;
    float s[2] = {0.f, 0.f};                                         // sum of the plane, sum of d glob over V
    MaxArg m[1] = {max_init()};
    for (int i = tid; i < a.hw; i += MM_ENC_BLOCK) {
        const float v = ld_px(a, xp, i);
        s[0] += v;
        m[0] = max_first(m[0], MaxArg{v, i});
    }
    for (int v = tid; v < a.V; v += MM_ENC_BLOCK) {
        float d = gL[v];
        for (int k = 0; k < a.row_k; ++k) {
            const int u = a.row_idx[(size_t)k * V + v];
            if (u >= 0) d += a.row_val[(size_t)k * V + v] * gN[u];
        }
        lds[v] = d;
        s[1] += gG[v];
    }
    block_reduce<2, 1>(s, m, red);
    const float w = sigmoidf_(a.p0[0]), mean = s[0] / (float)a.hw, dg = s[1];
    if (tid == 0 && a.part) a.part[bc] = dg * (m[0].v - mean);
    if (!a.gx) return;
    const float mean_share = dg * (1.f - w) / (float)a.hw, max_share = dg * w;
    const int amax = m[0].i;
    gather_pixels<T>(a, bc, lds, [&](int p, float acc) { acc += mean_share; return p == amax ? acc + max_share : acc; });
}

// ---- camera features --------------------------------------------------------------------------------------------------------
// the reductions of one plane: the 2x2 bins of x (sums s[0..3], maxima m[0..3]) and the two vertex bins of the sampled (V,1) map
// (sums s[4..5], maxima m[4..5]); the sampled row is not kept
template <typename T>
__device__ inline void camera_stats(const EncArgs& a, const T* xp, float* plane, float (&s)[6], MaxArg (&m)[6], float* red) {
    MM_FP_EXACT
    const int tid = threadIdx.x;
    int r0[2], r1[2], c0[2], c1[2], v0[2], v1[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        r0[i] = bin_lo(i, a.H, 2); r1[i] = bin_hi(i, a.H, 2);
        c0[i] = bin_lo(i, a.W, 2); c1[i] = bin_hi(i, a.W, 2);
        v0[i] = bin_lo(i, a.V, 2); v1[i] = bin_hi(i, a.V, 2);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) { s[k] = 0.f; m[k] = max_init(); }
    for (int i = tid; i < a.hw; i += MM_ENC_BLOCK) {
        const float v = ld_px(a, xp, i);
        if (plane) plane[i] = v;
        const int y = i / a.W, xx = i - y * a.W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int bi = k >> 1, bj = k & 1;
            if (y >= r0[bi] && y < r1[bi] && xx >= c0[bj] && xx < c1[bj]) { s[k] += v; m[k] = max_first(m[k], MaxArg{v, i}); }
        }
    }
    __syncthreads();
    for (int v = tid; v < a.V; v += MM_ENC_BLOCK) {
        const float l = sample_vertex(a, xp, plane, v);
#pragma unroll
        for (int r = 0; r < 2; ++r)
            if (v >= v0[r] && v < v1[r]) { s[4 + r] += l; m[4 + r] = max_first(m[4 + r], MaxArg{l, v}); }
    }
    block_reduce<6, 6>(s, m, red);
}

__device__ inline float bin_count(int i, int j, int H, int W) {
    return (float)((bin_hi(i, H, 2) - bin_lo(i, H, 2)) * (bin_hi(j, W, 2) - bin_lo(j, W, 2)));
}

template <typename T>
__global__ __launch_bounds__(MM_ENC_BLOCK) void camera_fwd_kernel(EncArgs a) {
    MM_FP_EXACT
    extern __shared__ float lds[];                                   // the staged plane
    __shared__ float red[MM_ENC_WAVES * 18];
    const int bc = blockIdx.x, b = bc / a.C, c = bc - b * a.C;
    const T* xp = (const T*)a.x + b * a.s0 + c * a.s1;
    float s[6];
    MaxArg m[6];
    camera_stats(a, xp, a.hw <= MM_ENC_PLANE_LDS ? lds : nullptr, s, m, red);
    if (threadIdx.x != 0) return;
    const float wm = sigmoidf_(a.p0[0]), wl = sigmoidf_(a.p1[0]);
    float* om = a.out + ((size_t)b * 2 * a.C + c) * 4;               // MMPool((2,2))(x)
    float* ol = a.out + ((size_t)b * 2 * a.C + a.C + c) * 4;         // MMPool((2,2)) of the (V,1) map: both columns are bin [0, 1)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int bi = k >> 1;
        om[k] = m[k].v * wm + (s[k] / bin_count(bi, k & 1, a.H, a.W)) * (1.f - wm);
        const float cnt = (float)(bin_hi(bi, a.V, 2) - bin_lo(bi, a.V, 2));
        ol[k] = m[4 + bi].v * wl + (s[4 + bi] / cnt) * (1.f - wl);
    }
}

template <typename T>
__global__ __launch_bounds__(MM_ENC_BLOCK) void camera_bwd_kernel(EncArgs a) {
    MM_FP_EXACT
    extern __shared__ float lds[];                                   // [V] d local, then the staged plane
    __shared__ float red[MM_ENC_WAVES * 18];
    const int bc = blockIdx.x, b = bc / a.C, c = bc - b * a.C, tid = threadIdx.x;
    const T* xp = (const T*)a.x + b * a.s0 + c * a.s1;
    float s[6];
    MaxArg m[6];
    camera_stats(a, xp, a.hw <= MM_ENC_PLANE_LDS ? lds + a.V : nullptr, s, m, red);
    const float* gm = a.g + ((size_t)b * 2 * a.C + c) * 4;           // (2,2) of the pool over x
    const float* gl = a.g + ((size_t)b * 2 * a.C + a.C + c) * 4;     // (2,2) of the pool over the (V,1) map
    const float wm = sigmoidf_(a.p0[0]), wl = sigmoidf_(a.p1[0]);
    float GL[2], lcnt[2], cnt[4];
    int v0[2], v1[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        GL[r] = gl[2 * r] + gl[2 * r + 1];                           // the two column bins coincide
        v0[r] = bin_lo(r, a.V, 2); v1[r] = bin_hi(r, a.V, 2);
        lcnt[r] = (float)(v1[r] - v0[r]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt[k] = bin_count(k >> 1, k & 1, a.H, a.W);
    if (tid == 0 && a.part) {
        float pm = 0.f, pl = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) pm += gm[k] * (m[k].v - s[k] / cnt[k]);
#pragma unroll
        for (int r = 0; r < 2; ++r) pl += GL[r] * (m[4 + r].v - s[4 + r] / lcnt[r]);
        a.part[bc] = pm;
        a.part[(size_t)a.B * a.C + bc] = pl;
    }
    if (!a.gx) return;
    for (int v = tid; v < a.V; v += MM_ENC_BLOCK) {
        float d = 0.f;
#pragma unroll
        for (int r = 0; r < 2; ++r)
            if (v >= v0[r] && v < v1[r]) {
                d += GL[r] * (1.f - wl) / lcnt[r];
                if (v == m[4 + r].i) d += GL[r] * wl;
            }
        lds[v] = d;
    }
    __syncthreads();
    int r0[2], r1[2], c0[2], c1[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        r0[i] = bin_lo(i, a.H, 2); r1[i] = bin_hi(i, a.H, 2);
        c0[i] = bin_lo(i, a.W, 2); c1[i] = bin_hi(i, a.W, 2);
    }
    gather_pixels<T>(a, bc, lds, [&](int p, float acc) {
        const int y = p / a.W, xx = p - y * a.W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int bi = k >> 1, bj = k & 1;
            if (y >= r0[bi] && y < r1[bi] && xx >= c0[bj] && xx < c1[bj]) {
                acc += gm[k] * (1.f - wm) / cnt[k];
                if (p == m[k].i) acc += gm[k] * wm;
            }
        }
        return acc;
    });
}

// ---- the per-pixel tap list: off (hw+1), then (vertex, weight) entries ordered by pixel, then vertex --------------------------
// one wave per pixel walks the vertices 64 at a time; a vertex has at most one tap on a given pixel (its four taps are distinct)
template <bool FILL>
__global__ __launch_bounds__(MM_ENC_BLOCK) void pix_list_kernel(EncArgs a, int* off, int* pv, float* pw) {
    const int p = blockIdx.x * MM_ENC_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= a.hw) return;                                           // wave-uniform
    int n = FILL ? off[p] : 0;
    for (int v0 = 0; v0 < a.V; v0 += 64) {
        const int v = v0 + lane;
        bool hit = false;
        float w = 0.f;
        if (v < a.V) {
            const Taps t = vertex_taps(a.tmpl, v, a.H, a.W, a.align);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t.idx[k] == p) { hit = true; w = t.w[k]; }
        }
        const uint64_t bal = __ballot(hit);
        if (FILL && hit) { const int e = n + ballot_rank(bal); pv[e] = v; pw[e] = w; }
        n += __popcll(bal);
    }
    if (!FILL && lane == 0) off[p] = n;
}

// counts -> exclusive offsets, in place; off[hw] = total.  One 1024-thread workgroup, a contiguous chunk per thread.
__global__ __launch_bounds__(1024) void pix_scan_kernel(int* off, int n) {
    __shared__ int sc[1024];
    const int t = threadIdx.x, per = (n + 1023) / 1024, lo = min(t * per, n), hi = min(lo + per, n);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += off[i];
    sc[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                             // inclusive Hillis-Steele scan
        const int add = t >= d ? sc[t - d] : 0;
        __syncthreads();
        sc[t] += add;
        __syncthreads();
    }
    int run = sc[t] - sum;
    for (int i = lo; i < hi; ++i) { const int k = off[i]; off[i] = run; run += k; }
    if (t == 1023) off[n] = sc[1023];
}

// grad p[k] = sigmoid'(p[k]) * sum over planes of part[k], summed in a fixed order.  One 1024-thread workgroup per p.
__global__ __launch_bounds__(1024) void dp_reduce_kernel(const float* part, int n, const float* p0, const float* p1, float* g0, float* g1) {
    MM_FP_EXACT
    __shared__ float red[16];
    const int k = blockIdx.x, t = threadIdx.x;
    float* dst = k == 0 ? g0 : g1;
    if (!dst) return;                                                // workgroup-uniform
    const float* src = part + (size_t)k * n;
    float s = 0.f;
    for (int i = t; i < n; i += 1024) s += src[i];
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
        float tot = red[0];
        for (int w = 1; w < 16; ++w) tot += red[w];
        const float y = sigmoidf_((k == 0 ? p0 : p1)[0]);
        dst[0] = tot * ((1.f - y) * y);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct PixList { int* off; int* pv; float* pw; float* part; size_t bytes; };

static PixList carve(void* base, int hw, int V, size_t planes, int nparts) {
    PixList l;
    char* p = (char*)base;
    size_t o = 0;
    l.off = (int*)(p + o); o += align256((size_t)(hw + 1) * 4);
    l.pv = (int*)(p + o); o += align256((size_t)4 * V * 4);
    l.pw = (float*)(p + o); o += align256((size_t)4 * V * 4);
    l.part = (float*)(p + o); o += align256((size_t)nparts * planes * 4);
    l.bytes = o;
    return l;
}

size_t encfeat_workspace_bytes(int B, int C, int H, int W, int V, int nparts) {
    return carve(nullptr, H * W, V, (size_t)B * C, nparts).bytes;
}

static EncArgs enc_args(int B, int C, int H, int W, int V, const void* x, const int64_t* st, const float* tmpl, bool align) {
    EncArgs a = {};
    a.B = B; a.C = C; a.H = H; a.W = W; a.V = V; a.hw = H * W;
    a.x = x; a.s0 = st[0]; a.s1 = st[1]; a.s2 = st[2]; a.s3 = st[3];
    a.tmpl = tmpl; a.align = align;
    // lanes per pixel of the backward's gather: about the mean list length (4V / hw taps at most), a power of two in 1..64
    const long long per = (4LL * V + a.hw - 1) / a.hw;
    a.group = 1;
    while (a.group < 64 && a.group < per) a.group <<= 1;
    return a;
}

static int build_pix_list(EncArgs& a, const PixList& l, hipStream_t s) {
    const dim3 grid((a.hw + MM_ENC_WAVES - 1) / MM_ENC_WAVES);
    hipLaunchKernelGGL(pix_list_kernel<false>, grid, dim3(MM_ENC_BLOCK), 0, s, a, l.off, l.pv, l.pw);
    hipLaunchKernelGGL(pix_scan_kernel, dim3(1), dim3(1024), 0, s, l.off, a.hw);
    hipLaunchKernelGGL(pix_list_kernel<true>, grid, dim3(MM_ENC_BLOCK), 0, s, a, l.off, l.pv, l.pw);
    a.pix_off = l.off; a.pix_v = l.pv; a.pix_w = l.pw;
    return launch_ok("encfeat pix_list");
}

#define MM_ENC_LAUNCH(kern, dtype, grid, lds_bytes, s, a)                                                                        \
    do {                                                                                                                         \
        if ((dtype) == MM_DTYPE_F16) hipLaunchKernelGGL(kern<_Float16>, grid, dim3(MM_ENC_BLOCK), lds_bytes, s, a);              \
        else if ((dtype) == MM_DTYPE_BF16) hipLaunchKernelGGL(kern<Bf16>, grid, dim3(MM_ENC_BLOCK), lds_bytes, s, a);            \
        else hipLaunchKernelGGL(kern<float>, grid, dim3(MM_ENC_BLOCK), lds_bytes, s, a);                                         \
    } while (0)

static size_t plane_lds(int hw) { return hw <= MM_ENC_PLANE_LDS ? (size_t)hw * 4 : 0; }

int launch_shape_feat_fwd(const MMShapeFeatDesc* d, hipStream_t s) {
    EncArgs a = enc_args(d->B, d->C, d->H, d->W, d->V, d->x, d->x_strides, d->template_xyz, true);
    a.col_k = d->col_k; a.col_idx = d->col_idx; a.col_val = d->col_val;
    a.p0 = d->p; a.out = d->out;
    MM_ENC_LAUNCH(shape_fwd_kernel, d->x_dtype, dim3(d->B * d->C), (size_t)d->V * 4 + plane_lds(a.hw), s, a);
    return launch_ok("shape_features_fwd");
}

int launch_shape_feat_bwd(const MMShapeFeatDesc* d, const MMShapeFeatGrads* g, hipStream_t s) {
    EncArgs a = enc_args(d->B, d->C, d->H, d->W, d->V, d->x, d->x_strides, d->template_xyz, true);
    a.row_k = d->row_k; a.row_idx = d->row_idx; a.row_val = d->row_val;
    a.p0 = d->p; a.g = g->grad_out; a.gx = g->grad_x;
    const PixList l = carve(d->workspace, a.hw, d->V, (size_t)d->B * d->C, 1);
    a.part = g->grad_p ? l.part : nullptr;
    if (a.gx && build_pix_list(a, l, s) != MM_OK) return MM_ERR_LAUNCH;
    MM_ENC_LAUNCH(shape_bwd_kernel, d->x_dtype, dim3(d->B * d->C), (size_t)d->V * 4, s, a);
    if (g->grad_p) hipLaunchKernelGGL(dp_reduce_kernel, dim3(1), dim3(1024), 0, s, l.part, d->B * d->C, d->p, d->p, g->grad_p, (float*)nullptr);
    return launch_ok("shape_features_bwd");
}

int launch_camera_feat_fwd(const MMCameraFeatDesc* d, hipStream_t s) {
    EncArgs a = enc_args(d->B, d->C, d->H, d->W, d->V, d->x, d->x_strides, d->template_xyz, false);
    a.p0 = d->p_map; a.p1 = d->p_local; a.out = d->out;
    MM_ENC_LAUNCH(camera_fwd_kernel, d->x_dtype, dim3(d->B * d->C), plane_lds(a.hw), s, a);
    return launch_ok("camera_features_fwd");
}

int launch_camera_feat_bwd(const MMCameraFeatDesc* d, const MMCameraFeatGrads* g, hipStream_t s) {
    EncArgs a = enc_args(d->B, d->C, d->H, d->W, d->V, d->x, d->x_strides, d->template_xyz, false);
    a.p0 = d->p_map; a.p1 = d->p_local; a.g = g->grad_out; a.gx = g->grad_x;
    const PixList l = carve(d->workspace, a.hw, d->V, (size_t)d->B * d->C, 2);
    const bool want_p = g->grad_p_map || g->grad_p_local;
    a.part = want_p ? l.part : nullptr;
    if (a.gx && build_pix_list(a, l, s) != MM_OK) return MM_ERR_LAUNCH;
    MM_ENC_LAUNCH(camera_bwd_kernel, d->x_dtype, dim3(d->B * d->C), (size_t)d->V * 4 + plane_lds(a.hw), s, a);
    if (want_p)
        hipLaunchKernelGGL(dp_reduce_kernel, dim3(2), dim3(1024), 0, s, l.part, d->B * d->C, d->p_map, d->p_local, g->grad_p_map, g->grad_p_local);
    return launch_ok("camera_features_bwd");
}

}  // namespace mm
