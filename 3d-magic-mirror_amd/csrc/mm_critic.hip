// mm_critic.hip -- the image batches the discriminator sees in the reference's GAN step, for gfx950 (trainer.py:370-411, 429-431).
//
// Replaces, per iteration: three compositions over white (smr_utils.py:198-202), three detach().clone() copies and a cat for the D
// step, two gradient-penalty interpolates (smr_utils.py:340-346) and a second cat for the G step -- and the strided gathers that turn
// the renders' NHWC memory into the NCHW batches a convolution wants.  With M the channel map of the unmask mode
//   unmask 0 (C = 3): M(X)_c = fl(fl(X_c * m) + fl(1 - m)),  m = X_3
//   unmask 1 (C = 3): M(X)_c = X_c
//   unmask 2 (C = 4): M(X)   = X
// critic_fwd writes out_batch (3B,C,H,W) = cat(M(Xa), M(Xer90), M(Xir)) -- whose rows [B, 3B) are the G step's batch -- and, when the
// alphas are given, gp_j (B,C,H,W) = fl(fl(a_j * M(Xa)) + fl(fl(1 - a_j) * M(X_j))): torch's eager fp32 results bit for bit (the file
// is compiled without contraction).  critic_bwd turns the (2B,C,H,W) gradient of rows [B, 3B) into the gradients of Xer90 and Xir,
// each written with its input's own layout:
//   unmask 0: d X_c = fl(g_c * m),  d m = ((g_0 * (X_0 - 1)) + g_1 * (X_1 - 1)) + g_2 * (X_2 - 1)
//   unmask 1: d X_c = g_c, d m = 0;      unmask 2: d X = g
// Both are pure streams: no LDS, no scratch, no atomics, every output element written by one lane (bitwise reproducible).  The work is
// cut into chunks of MM_CRITIC_BLOCK * 4 pixels of ONE image, so the image index and its two alphas are wave-uniform; a grid of at
// most MM_CRITIC_GRID workgroups strides over the chunks.  A lane owns four consecutive pixels: an NHWC input is four 16-byte loads
// of 64 contiguous bytes, an NCHW input one 16-byte load per plane, every output plane one 16-byte store.  H * W not a multiple of 4,
// or a base address off a 16-byte boundary, takes the PX = 1 instantiation (one pixel per lane, 4-byte accesses).  Offsets are 64-bit.
// Plain stores: the next kernel (the critic's first convolution) reads the batch.
#include <hip/hip_runtime.h>

#include "mm_device.h"

#define MM_CRITIC_BLOCK 256
#define MM_CRITIC_GRID 2048                                   // 256 CUs x 8 workgroups (cdna_hip_programming.md, Guideline 11)

namespace mm {

struct CriticFwdArgs {
    const float* x[3];                                        // Xa, Xer90, Xir: (B,4,H,W)
    int nhwc[3];                                              // 1: strides (4HW, 1, 4W, 4); 0: NCHW-contiguous
    const float* alpha[2];                                    // (B) each, or both NULL
    float* out;                                               // (3B,C,H,W)
    float* gp[2];                                             // (B,C,H,W) each, read only with the alphas
    int B, nchunk;
    long long HW;
};

struct CriticBwdArgs {
    const float* x[2];                                        // the fakes (read by unmask 0 only)
    const float* g[2];                                        // rows of the (2B,C,H,W) upstream gradient: image b of fake j at g[j] + b*C*HW
    float* dx[2];                                             // (B,4,H,W) in the layout of dnhwc
    int xnhwc[2], dnhwc[2];
    int n;                                                    // fakes that take a gradient (1 or 2)
    int B, nchunk;
    long long HW;
};

// V: what a lane holds of one plane -- float4 (four consecutive pixels, PX = 4) or float (one pixel, PX = 1).  Img: the four planes.
template <typename V> struct Img { V c0, c1, c2, c3; };
template <int PX> struct LaneOf { typedef float V; };
template <> struct LaneOf<4> { typedef float4 V; };

__device__ inline float splat(float, float s) { return s; }
__device__ inline float4 splat(float4, float s) { return make_float4(s, s, s, s); }
__device__ inline float mul(float a, float b) { MM_FP_EXACT return a * b; }
__device__ inline float4 mul(float4 a, float4 b) { MM_FP_EXACT return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ inline float add(float a, float b) { MM_FP_EXACT return a + b; }
__device__ inline float4 add(float4 a, float4 b) { MM_FP_EXACT return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline float sub(float a, float b) { MM_FP_EXACT return a - b; }
__device__ inline float4 sub(float4 a, float4 b) { MM_FP_EXACT return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// planes [0, NCH) of the lane's pixels of image b, from pixel p on.  Either layout is four 16-byte loads at base + k * step: an NHWC
// input's four pixels (64 contiguous bytes, whatever NCH is; transposed in registers), an NCHW input's four planes (the last one only
// for NCH = 4).  One address form for both keeps the loads whole: two branches with loads of their own get merged element by element.
// Raw4 is what the loads return; planes() sorts it into planes.
struct Raw4 { float4 t0, t1, t2, t3; };
template <int NCH>
__device__ inline Raw4 load_raw(const float* __restrict__ x, int nhwc, long long b, long long HW, long long p) {
    const float* q = x + (nhwc ? (b * HW + p) * 4 : b * 4 * HW + p);
    const long long step = nhwc ? 4 : HW;
    Raw4 r;
    r.t0 = *(const float4*)q; r.t1 = *(const float4*)(q + step); r.t2 = *(const float4*)(q + 2 * step);
    r.t3 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (NCH == 4 || nhwc) r.t3 = *(const float4*)(q + 3 * step);
    return r;
}
// says that all four components of v are read: without it, a mode that needs no alpha (unmask 1) has the compiler cut an NHWC pixel's
// load into 12 + 4 bytes.  No instruction; placed after every load of the iteration has been issued.
__device__ inline void whole(float4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
__device__ inline void whole(Raw4& r) { whole(r.t0); whole(r.t1); whole(r.t2); whole(r.t3); }
__device__ inline Img<float4> planes(const Raw4& r, int nhwc) {
    Img<float4> o;
    o.c0 = nhwc ? make_float4(r.t0.x, r.t1.x, r.t2.x, r.t3.x) : r.t0; o.c1 = nhwc ? make_float4(r.t0.y, r.t1.y, r.t2.y, r.t3.y) : r.t1;
    o.c2 = nhwc ? make_float4(r.t0.z, r.t1.z, r.t2.z, r.t3.z) : r.t2; o.c3 = nhwc ? make_float4(r.t0.w, r.t1.w, r.t2.w, r.t3.w) : r.t3;
    return o;
}
template <int NCH>
__device__ inline Img<float4> load_image(float4, const float* __restrict__ x, int nhwc, long long b, long long HW, long long p) {
    return planes(load_raw<NCH>(x, nhwc, b, HW, p), nhwc);
}
template <int NCH>
__device__ inline Img<float> load_image(float, const float* __restrict__ x, int nhwc, long long b, long long HW, long long p) {
    Img<float> r;
    if (nhwc) {
        const float* q = x + (b * HW + p) * 4;
        r.c0 = q[0]; r.c1 = q[1]; r.c2 = q[2]; r.c3 = q[3];
    } else {
        const float* q = x + b * 4 * HW + p;
        r.c0 = q[0]; r.c1 = q[HW]; r.c2 = q[2 * HW];
        if constexpr (NCH == 4) r.c3 = q[3 * HW]; else r.c3 = 0.f;
    }
    return r;
}

// the store twin of load_raw: four 16-byte stores at base + k * step in either layout
__device__ inline void store_image(float* __restrict__ x, int nhwc, long long b, long long HW, long long p, const Img<float4>& d) {
    float* q = x + (nhwc ? (b * HW + p) * 4 : b * 4 * HW + p);
    const long long step = nhwc ? 4 : HW;
    *(float4*)q = nhwc ? make_float4(d.c0.x, d.c1.x, d.c2.x, d.c3.x) : d.c0;
    *(float4*)(q + step) = nhwc ? make_float4(d.c0.y, d.c1.y, d.c2.y, d.c3.y) : d.c1;
    *(float4*)(q + 2 * step) = nhwc ? make_float4(d.c0.z, d.c1.z, d.c2.z, d.c3.z) : d.c2;
    *(float4*)(q + 3 * step) = nhwc ? make_float4(d.c0.w, d.c1.w, d.c2.w, d.c3.w) : d.c3;
}
__device__ inline void store_image(float* __restrict__ x, int nhwc, long long b, long long HW, long long p, const Img<float>& d) {
    if (nhwc) {
        float* q = x + (b * HW + p) * 4;
        q[0] = d.c0; q[1] = d.c1; q[2] = d.c2; q[3] = d.c3;
    } else {
        float* q = x + b * 4 * HW + p;
        q[0] = d.c0; q[HW] = d.c1; q[2 * HW] = d.c2; q[3 * HW] = d.c3;
    }
}

// C planes of an NCHW image whose plane 0 starts at q
template <int C, typename V>
__device__ inline void store_planes(float* __restrict__ q, long long HW, const Img<V>& v) {
    *(V*)q = v.c0; *(V*)(q + HW) = v.c1; *(V*)(q + 2 * HW) = v.c2;
    if constexpr (C == 4) *(V*)(q + 3 * HW) = v.c3;
}

// the channel map M
template <int UNMASK, typename V>
__device__ inline Img<V> channel_map(const Img<V>& x) {
    if constexpr (UNMASK != 0) return x;
    else {
        const V w = sub(splat(x.c3, 1.0f), x.c3);             // fl(1 - m)
        Img<V> r;
        r.c0 = add(mul(x.c0, x.c3), w); r.c1 = add(mul(x.c1, x.c3), w); r.c2 = add(mul(x.c2, x.c3), w); r.c3 = x.c3;
        return r;
    }
}

// fl(fl(a * real) + fl(om * fake)), om = fl(1 - a)
template <typename V>
__device__ inline Img<V> penalty_mix(float a, float om, const Img<V>& real, const Img<V>& fake) {
    const V va = splat(real.c0, a), vo = splat(real.c0, om);
    Img<V> r;
    r.c0 = add(mul(va, real.c0), mul(vo, fake.c0)); r.c1 = add(mul(va, real.c1), mul(vo, fake.c1));
    r.c2 = add(mul(va, real.c2), mul(vo, fake.c2)); r.c3 = add(mul(va, real.c3), mul(vo, fake.c3));
    return r;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// alpha_er90 / alpha_ir are parameters of their own: read-only and unaliased, so their wave-uniform loads stay scalar loads
template <int UNMASK, int PX>
__global__ __launch_bounds__(MM_CRITIC_BLOCK) void critic_fwd_kernel(CriticFwdArgs a, const float* __restrict__ alpha_er90,
                                                                     const float* __restrict__ alpha_ir) {
    MM_FP_EXACT
    typedef typename LaneOf<PX>::V V;
    constexpr int C = UNMASK == 2 ? 4 : 3;
    constexpr int NCH = UNMASK == 1 ? 3 : 4;                  // planes an NCHW input is read for
    const long long HW = a.HW;
    const int total = a.B * a.nchunk;
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int b = item / a.nchunk, chunk = item - b * a.nchunk;
        const long long p = ((long long)chunk * MM_CRITIC_BLOCK + threadIdx.x) * PX;
        if (p >= HW) continue;                                // (HW % PX == 0: a lane's pixels are all inside or all outside)
        Img<V> xa, x1, x2;
        if constexpr (PX == 4 && UNMASK == 1) {
            Raw4 ra = load_raw<NCH>(a.x[0], a.nhwc[0], b, HW, p), r1 = load_raw<NCH>(a.x[1], a.nhwc[1], b, HW, p);
            Raw4 r2 = load_raw<NCH>(a.x[2], a.nhwc[2], b, HW, p);
            whole(ra); whole(r1); whole(r2);
            xa = planes(ra, a.nhwc[0]); x1 = planes(r1, a.nhwc[1]); x2 = planes(r2, a.nhwc[2]);
        } else {
            xa = load_image<NCH>(V(), a.x[0], a.nhwc[0], b, HW, p);
            x1 = load_image<NCH>(V(), a.x[1], a.nhwc[1], b, HW, p);
            x2 = load_image<NCH>(V(), a.x[2], a.nhwc[2], b, HW, p);
        }
        const Img<V> ma = channel_map<UNMASK>(xa), m1 = channel_map<UNMASK>(x1), m2 = channel_map<UNMASK>(x2);
        const long long img = (long long)C * HW;              // floats per output image
        store_planes<C>(a.out + (long long)b * img + p, HW, ma);
        store_planes<C>(a.out + ((long long)a.B + b) * img + p, HW, m1);
        store_planes<C>(a.out + (2LL * a.B + b) * img + p, HW, m2);
        if (alpha_er90) {
            const float a1 = alpha_er90[b], a2 = alpha_ir[b];
            store_planes<C>(a.gp[0] + (long long)b * img + p, HW, penalty_mix(a1, 1.0f - a1, ma, m1));
            store_planes<C>(a.gp[1] + (long long)b * img + p, HW, penalty_mix(a2, 1.0f - a2, ma, m2));
        }
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
template <int UNMASK, int PX>
__global__ __launch_bounds__(MM_CRITIC_BLOCK) void critic_bwd_kernel(CriticBwdArgs a) {
    MM_FP_EXACT
    typedef typename LaneOf<PX>::V V;
    constexpr int C = UNMASK == 2 ? 4 : 3;
    const long long HW = a.HW;
    const int per = a.B * a.nchunk, total = a.n * per;
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const bool j = item >= per;                           // which fake: selects, not indexed loads of the arguments
        const int r = j ? item - per : item;
        const int b = r / a.nchunk, chunk = r - b * a.nchunk;
        const long long p = ((long long)chunk * MM_CRITIC_BLOCK + threadIdx.x) * PX;
        if (p >= HW) continue;
        const float* gq = (j ? a.g[1] : a.g[0]) + (long long)b * C * HW + p;
        Img<V> g, d;
        g.c0 = *(const V*)gq; g.c1 = *(const V*)(gq + HW); g.c2 = *(const V*)(gq + 2 * HW);
        if constexpr (C == 4) g.c3 = *(const V*)(gq + 3 * HW); else g.c3 = splat(g.c0, 0.0f);
        if constexpr (UNMASK == 0) {
            const Img<V> x = load_image<4>(V(), j ? a.x[1] : a.x[0], j ? a.xnhwc[1] : a.xnhwc[0], b, HW, p);
            const V one = splat(g.c0, 1.0f);
            d.c0 = mul(g.c0, x.c3); d.c1 = mul(g.c1, x.c3); d.c2 = mul(g.c2, x.c3);
            d.c3 = add(add(mul(g.c0, sub(x.c0, one)), mul(g.c1, sub(x.c1, one))), mul(g.c2, sub(x.c2, one)));
        } else {
            d = g;                                            // unmask 1: d m = 0 (g.c3 above); unmask 2: the identity
        }
        store_image(j ? a.dx[1] : a.dx[0], j ? a.dnhwc[1] : a.dnhwc[0], b, HW, p, d);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static int critic_chunks(long long HW, int px) { return (int)((HW + (long long)MM_CRITIC_BLOCK * px - 1) / ((long long)MM_CRITIC_BLOCK * px)); }
static dim3 critic_grid(long long total) { return dim3((unsigned)(total < MM_CRITIC_GRID ? total : MM_CRITIC_GRID)); }
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// chunks of one image for the descriptor's shape in the path its pointers allow (the entry point checks B * chunks against int32)
int critic_chunks_per_image(const MMCriticDesc* d) { return critic_chunks((long long)d->H * d->W, 1); }

template <int UNMASK>
static void launch_fwd_t(const CriticFwdArgs& a, bool vec, hipStream_t s) {
    const dim3 grid = critic_grid((long long)a.B * a.nchunk);
    if (vec) hipLaunchKernelGGL((critic_fwd_kernel<UNMASK, 4>), grid, dim3(MM_CRITIC_BLOCK), 0, s, a, a.alpha[0], a.alpha[1]);
    else hipLaunchKernelGGL((critic_fwd_kernel<UNMASK, 1>), grid, dim3(MM_CRITIC_BLOCK), 0, s, a, a.alpha[0], a.alpha[1]);
}

template <int UNMASK>
static void launch_bwd_t(const CriticBwdArgs& a, bool vec, hipStream_t s) {
    const dim3 grid = critic_grid((long long)a.n * a.B * a.nchunk);
    if (vec) hipLaunchKernelGGL((critic_bwd_kernel<UNMASK, 4>), grid, dim3(MM_CRITIC_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((critic_bwd_kernel<UNMASK, 1>), grid, dim3(MM_CRITIC_BLOCK), 0, s, a);
}

int launch_critic_fwd(const MMCriticDesc* d, hipStream_t s) {
    CriticFwdArgs a = {};
    a.x[0] = d->Xa; a.x[1] = d->Xer90; a.x[2] = d->Xir;
    a.nhwc[0] = d->Xa_nhwc != 0; a.nhwc[1] = d->Xer90_nhwc != 0; a.nhwc[2] = d->Xir_nhwc != 0;
    a.alpha[0] = d->alpha_er90; a.alpha[1] = d->alpha_ir;
    a.out = d->out_batch; a.gp[0] = d->out_gp_er90; a.gp[1] = d->out_gp_ir;
    a.B = d->B; a.HW = (long long)d->H * d->W;
    bool vec = a.HW % 4 == 0 && aligned16(a.x[0]) && aligned16(a.x[1]) && aligned16(a.x[2]) && aligned16(a.out);
    if (a.alpha[0]) vec = vec && aligned16(a.gp[0]) && aligned16(a.gp[1]);
    a.nchunk = critic_chunks(a.HW, vec ? 4 : 1);
    switch (d->unmask) {
        case 0: launch_fwd_t<0>(a, vec, s); break;
        case 1: launch_fwd_t<1>(a, vec, s); break;
        default: launch_fwd_t<2>(a, vec, s); break;
    }
    return launch_ok("critic_fwd");
}

int launch_critic_bwd(const MMCriticDesc* d, const MMCriticGrads* g, hipStream_t s) {
    CriticBwdArgs a = {};
    const int C = d->unmask == 2 ? 4 : 3;
    a.B = d->B; a.HW = (long long)d->H * d->W;
    const float* x[2] = {d->Xer90, d->Xir};
    const int xl[2] = {d->Xer90_nhwc != 0, d->Xir_nhwc != 0};
    float* dx[2] = {g->grad_er90, g->grad_ir};
    const int dl[2] = {g->grad_er90_nhwc != 0, g->grad_ir_nhwc != 0};
    bool vec = a.HW % 4 == 0 && aligned16(g->g_batch);
    for (int j = 0; j < 2; ++j) {
        if (!dx[j]) continue;
        a.x[a.n] = x[j]; a.xnhwc[a.n] = xl[j]; a.dx[a.n] = dx[j]; a.dnhwc[a.n] = dl[j];
        a.g[a.n] = g->g_batch + (long long)j * d->B * C * a.HW;
        vec = vec && aligned16(dx[j]) && (d->unmask != 0 || aligned16(x[j]));
        ++a.n;
    }
    if (a.n == 0) return MM_OK;                               // neither fake takes a gradient: nothing to launch
    a.nchunk = critic_chunks(a.HW, vec ? 4 : 1);
    switch (d->unmask) {
        case 0: launch_bwd_t<0>(a, vec, s); break;
        case 1: launch_bwd_t<1>(a, vec, s); break;
        default: launch_bwd_t<2>(a, vec, s); break;
    }
    return launch_ok("critic_bwd");
}

}  // namespace mm
