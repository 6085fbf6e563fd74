// mm_disentangle.hip -- the disentangle regularisation of the generator step for gfx950 (--dis1 / --dis2, trainer.py:455-494).
//
// Two pieces.  (1) disentangle_inputs: the two extra encoder batches, fliplr(Xa) and RandomErasing(p=1)(Xa), in ONE launch -- every input
// element read once, every output element written once, 16 bytes per lane where the pointers and W allow it.  (2) the seven terms, the
// sibling of mm_attloss.hip: l_text = mean |fliplr(Tf) - T| with Tf read mirrored (no mirrored copy), two means of per-sample L2 norms of
// vertex differences (one with x negated), four small camera means through angle2xy -- one streaming launch forward (fixed-order partials,
// the last workgroup adds them up and takes the square roots: no float atomics, the same bits run to run) and one launch for every gradient
// of BOTH attribute sets, each element written exactly once.
#include "mm_device.h"

namespace mm {

// ---- (1) the encoder inputs ----------------------------------------------------------------------------------------------------------

struct DisInArgs {
    int B, C, H, W, nhwc;
    int bi, bj, bh, bw;              // the batch's one box (i, j, h, w), used when boxes == nullptr
    float value;
    const float* x;
    const int* boxes;                // (B,4) rows (i, j, h, w), or nullptr
    int boxes16;                     // boxes is 16-byte aligned: a row is one 16-byte load
    float* out_flip;                 // NCHW, or nullptr
    float* out_erase;                // NCHW, or nullptr
};

// the box of sample b clamped to the image: rows [y0, y1), columns [x0, x1) (empty when h or w is < 1 or the box lies outside)
struct DisBox { int y0, y1, x0, x1; };
__device__ inline int dis_clamp(long long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }
__device__ inline DisBox dis_box(const DisInArgs& a, int b) {
    int i = a.bi, j = a.bj, h = a.bh, w = a.bw;
    if (a.boxes && a.boxes16) { const int4 q = ((const int4*)a.boxes)[b]; i = q.x; j = q.y; h = q.z; w = q.w; }
    else if (a.boxes) { i = a.boxes[b * 4]; j = a.boxes[b * 4 + 1]; h = a.boxes[b * 4 + 2]; w = a.boxes[b * 4 + 3]; }
    DisBox r;
    r.y0 = dis_clamp(i, 0, a.H); r.y1 = dis_clamp((long long)i + h, r.y0, a.H);
    r.x0 = dis_clamp(j, 0, a.W); r.x1 = dis_clamp((long long)j + w, r.x0, a.W);
    return r;
}
__device__ inline float dis_erased(float v, const DisBox& k, int y, int x, float value) {
    return (y >= k.y0 && y < k.y1 && x >= k.x0 && x < k.x1) ? value : v;
}

// scalar form, any layout, any alignment: one thread per element, indexed as the NCHW outputs are
__global__ __launch_bounds__(256) void dis_inputs_scalar_kernel(DisInArgs a) {
    const unsigned n = (unsigned)a.B * a.C * a.H * a.W;
    const unsigned o = blockIdx.x * 256u + threadIdx.x;
    if (o >= n) return;
    const unsigned x = o % (unsigned)a.W, row = o / (unsigned)a.W;          // row = (b * C + c) * H + y
    const unsigned y = row % (unsigned)a.H, bc = row / (unsigned)a.H;
    const unsigned c = bc % (unsigned)a.C, b = bc / (unsigned)a.C;
    const size_t src = a.nhwc ? (((size_t)b * a.H + y) * a.W + x) * a.C + c : (size_t)o;
    const float v = a.x[src];
    if (a.out_flip) a.out_flip[(size_t)row * a.W + (a.W - 1 - x)] = v;
    if (a.out_erase) a.out_erase[o] = dis_erased(v, dis_box(a, (int)b), (int)y, (int)x, a.value);
}

// NCHW, W % 4 == 0, every pointer 16-byte aligned: one thread per four columns of one row
__global__ __launch_bounds__(256) void dis_inputs_nchw4_kernel(DisInArgs a) {
    const unsigned wq = (unsigned)a.W >> 2;
    const unsigned n4 = (unsigned)a.B * a.C * a.H * wq;
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n4) return;
    const unsigned xq = q % wq, row = q / wq;
    const float4 v = ((const float4*)a.x)[q];
    if (a.out_flip) ((float4*)a.out_flip)[row * wq + (wq - 1 - xq)] = make_float4(v.w, v.z, v.y, v.x);
    if (a.out_erase) {
        const int y = (int)(row % (unsigned)a.H), b = (int)(row / ((unsigned)a.H * a.C)), x = (int)(xq << 2);
        const DisBox k = dis_box(a, b);
        ((float4*)a.out_erase)[q] = make_float4(dis_erased(v.x, k, y, x, a.value), dis_erased(v.y, k, y, x + 1, a.value),
                                               dis_erased(v.z, k, y, x + 2, a.value), dis_erased(v.w, k, y, x + 3, a.value));
    }
}

// NHWC, C = 3 or 4, W % 4 == 0, every pointer 16-byte aligned: one thread per four pixels of one image row -- C 16-byte loads of
// consecutive memory, C 16-byte stores per output (one per channel plane)
template <int C>
__global__ __launch_bounds__(256) void dis_inputs_nhwc4_kernel(DisInArgs a) {
    const unsigned wq = (unsigned)a.W >> 2;
    const unsigned n4 = (unsigned)a.B * a.H * wq;
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n4) return;
    const unsigned xq = q % wq, by = q / wq;                               // by = b * H + y
    const unsigned y = by % (unsigned)a.H, b = by / (unsigned)a.H;
    float v[4 * C];                                                        // v[p * C + c]: pixel p of the four, channel c
    const float4* src = (const float4*)a.x + (size_t)q * C;
#pragma unroll
    for (int k = 0; k < C; ++k) { const float4 t = src[k]; v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w; }
    const DisBox bx = dis_box(a, (int)b);
    const int x = (int)(xq << 2);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const size_t row = ((size_t)b * C + c) * a.H + y;
        if (a.out_flip) ((float4*)a.out_flip)[row * wq + (wq - 1 - xq)] = make_float4(v[3 * C + c], v[2 * C + c], v[C + c], v[c]);
        if (a.out_erase)
            ((float4*)a.out_erase)[row * wq + xq] = make_float4(dis_erased(v[c], bx, (int)y, x, a.value), dis_erased(v[C + c], bx, (int)y, x + 1, a.value),
                                                               dis_erased(v[2 * C + c], bx, (int)y, x + 2, a.value), dis_erased(v[3 * C + c], bx, (int)y, x + 3, a.value));
    }
}

int launch_disentangle_inputs(const MMDisentangleInputsDesc* d, hipStream_t s) {
    DisInArgs a;
    a.B = d->B; a.C = d->C; a.H = d->H; a.W = d->W; a.nhwc = d->nhwc != 0;
    a.bi = d->box[0]; a.bj = d->box[1]; a.bh = d->box[2]; a.bw = d->box[3];
    a.value = d->value; a.x = d->x; a.boxes = d->boxes; a.boxes16 = (((size_t)d->boxes) & 15) == 0; a.out_flip = d->out_flip; a.out_erase = d->out_erase;
    const size_t n = (size_t)d->B * d->C * d->H * d->W;
    const bool wide = (d->W & 3) == 0 && ((((size_t)d->x) | ((size_t)d->out_flip) | ((size_t)d->out_erase)) & 15) == 0;
    if (wide && !a.nhwc) {
        hipLaunchKernelGGL(dis_inputs_nchw4_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, a);
    } else if (wide && d->C == 4) {
        hipLaunchKernelGGL(dis_inputs_nhwc4_kernel<4>, dim3((unsigned)((n / 16 + 255) / 256)), dim3(256), 0, s, a);
    } else if (wide && d->C == 3) {
        hipLaunchKernelGGL(dis_inputs_nhwc4_kernel<3>, dim3((unsigned)((n / 12 + 255) / 256)), dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(dis_inputs_scalar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    }
    return launch_ok("disentangle_inputs");
}

// ---- (2) the seven terms ---------------------------------------------------------------------------------------------------------------

struct DisArgs {
    int B, V, Ht, Wt;
    const float *te, *ve, *az, *el, *di, *bi, *dv;                  // Ae
    const float *f_te, *f_ve;                                       // Ae_fliplr (both or neither)
    const float *j_az, *j_el, *j_di, *j_bi, *j_dv;                  // Ae_jitter (all or none)
    float* terms;                    // (7): text, shape_flip, azim, elev, dist, bias, shape_jitter
    float* partial;                  // (blocks) sums of |d| over a workgroup's texels
    float* cam;                      // (4) sums of the camera terms (workgroup 0)
    float* sq;                       // (B,2) per-sample sums of squares: flip, jitter
    float* norm;                     // (B,2) their square roots, left for the backward
    unsigned* ticket;
    const float* weights;            // (7) dL/d terms[k]
    float *g_te, *g_ve, *g_az, *g_el, *g_di, *g_bi, *g_dv;          // d/d Ae (any may be null)
    float *gf_te, *gf_ve;                                           // d/d Ae_fliplr
    float *gj_az, *gj_el, *gj_di, *gj_bi, *gj_dv;                   // d/d Ae_jitter
};

__device__ inline float dis_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
// can rows of Wt texels be walked in 16-byte pieces from these pointers?
__device__ inline bool dis_wide(int Wt, size_t pointers) { return (Wt & 3) == 0 && (pointers & 15) == 0; }

__global__ __launch_bounds__(256) void dis_fwd_kernel(DisArgs a) {
    __shared__ float s_red[4];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const unsigned gid = blockIdx.x * 256u + tid, gstride = gridDim.x * 256u;
    const unsigned rows = (unsigned)a.B * 3u * a.Ht;
    if (a.f_te) {                                                    // l_text: T in memory order, Tf mirrored along its rows
        float s = 0.f;
        if (dis_wide(a.Wt, ((size_t)a.te) | ((size_t)a.f_te))) {
            const float4* t4 = (const float4*)a.te; const float4* f4 = (const float4*)a.f_te;
            const unsigned wq = (unsigned)a.Wt >> 2, n4 = rows * wq;
            unsigned i = gid;
            for (; i + gstride < n4; i += 2 * gstride) {             // four 16-byte loads in flight per trip
                const unsigned j = i + gstride;
                const unsigned r0 = i / wq, r1 = j / wq;
                const float4 t0 = t4[i], t1 = t4[j];
                const float4 f0 = f4[r0 * wq + (wq - 1 - (i - r0 * wq))], f1 = f4[r1 * wq + (wq - 1 - (j - r1 * wq))];
                s += ((fabsf(f0.w - t0.x) + fabsf(f0.z - t0.y)) + fabsf(f0.y - t0.z)) + fabsf(f0.x - t0.w);
                s += ((fabsf(f1.w - t1.x) + fabsf(f1.z - t1.y)) + fabsf(f1.y - t1.z)) + fabsf(f1.x - t1.w);
            }
            for (; i < n4; i += gstride) {
                const unsigned r0 = i / wq;
                const float4 t0 = t4[i], f0 = f4[r0 * wq + (wq - 1 - (i - r0 * wq))];
                s += ((fabsf(f0.w - t0.x) + fabsf(f0.z - t0.y)) + fabsf(f0.y - t0.z)) + fabsf(f0.x - t0.w);
            }
        } else {
            const unsigned W = (unsigned)a.Wt, n = rows * W;
            for (unsigned i = gid; i < n; i += gstride) {
                const unsigned r = i / W;
                s += fabsf(a.f_te[r * W + (W - 1 - (i - r * W))] - a.te[i]);
            }
        }
        const float t = block_sum(s, s_red);
        if (tid == 0) publish_exchange(a.partial + blockIdx.x, t);
    }
    // the per-sample sums of squares: one workgroup per sample and term, its 3V differences strided over the threads
    const int n3 = a.V * 3;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        if (a.f_ve) {
            float s = 0.f;
            for (int i = tid; i < n3; i += 256) {
                const float v = a.ve[(size_t)b * n3 + i];
                const float d = a.f_ve[(size_t)b * n3 + i] - (i % 3 == 0 ? -v : v);
                s += d * d;
            }
            const float t = block_sum(s, s_red);
            if (tid == 0) publish_exchange(a.sq + b * 2, t);
        }
        if (a.j_dv) {
            float s = 0.f;
            for (int i = tid; i < n3; i += 256) { const float d = a.j_dv[(size_t)b * n3 + i] - a.dv[(size_t)b * n3 + i]; s += d * d; }
            const float t = block_sum(s, s_red);
            if (tid == 0) publish_exchange(a.sq + b * 2 + 1, t);
        }
    }
    if (blockIdx.x == 0 && a.j_dv) {                                  // the small ones: squared differences, angles through angle2xy
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int i = tid; i < a.B; i += 256) {
            const float pa = a.j_az[i] * MM_DEG2RAD, ta = a.az[i] * MM_DEG2RAD;
            const float dc = cosf(pa) - cosf(ta), ds = sinf(pa) - sinf(ta);
            s0 += dc * dc + ds * ds;
            const float pe = a.j_el[i] * MM_DEG2RAD, te = a.el[i] * MM_DEG2RAD;
            const float ec = cosf(pe) - cosf(te), es = sinf(pe) - sinf(te);
            s1 += ec * ec + es * es;
            const float dd = a.j_di[i] - a.di[i];
            s2 += dd * dd;
        }
        for (int i = tid; i < a.B * 2; i += 256) { const float d = a.j_bi[i] - a.bi[i]; s3 += d * d; }
        const float t0 = block_sum(s0, s_red), t1 = block_sum(s1, s_red), t2 = block_sum(s2, s_red), t3 = block_sum(s3, s_red);
        if (tid < 4) publish_exchange(a.cam + tid, tid == 0 ? t0 : (tid == 1 ? t1 : (tid == 2 ? t2 : t3)));
    }
    if (!last_workgroup(a.ticket, gridDim.x, true, s_last)) return;     // (the hand-off: mm_device.h)
    // the last workgroup: texture partials strided over its threads, the norms' square roots, then fixed-order block sums
    float at = 0.f, af = 0.f, aj = 0.f;
    if (a.f_te) {
        for (unsigned i = tid; i < gridDim.x; i += 256) at += __hip_atomic_load(a.partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int b = tid; b < a.B; b += 256) {
            const float r = sqrtf(__hip_atomic_load(a.sq + b * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            a.norm[b * 2] = r;
            af += r;
        }
    }
    if (a.j_dv) {
        for (int b = tid; b < a.B; b += 256) {
            const float r = sqrtf(__hip_atomic_load(a.sq + b * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            a.norm[b * 2 + 1] = r;
            aj += r;
        }
    }
    const float tt = block_sum(at, s_red), tf = block_sum(af, s_red), tj = block_sum(aj, s_red);
    if (tid != 0) return;
    const float Bf = (float)a.B;
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.j_dv) {
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = __hip_atomic_load(a.cam + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    a.terms[0] = a.f_te ? tt / (Bf * (float)(3 * a.Ht * a.Wt)) : 0.f;
    a.terms[1] = a.f_te ? tf / Bf : 0.f;
    a.terms[2] = c[0] / (Bf * 2.f);
    a.terms[3] = c[1] / (Bf * 2.f);
    a.terms[4] = c[2] / Bf;
    a.terms[5] = c[3] / (Bf * 2.f);
    a.terms[6] = a.j_dv ? tj / Bf : 0.f;
}

__global__ __launch_bounds__(256) void dis_bwd_kernel(DisArgs a) {
    const int tid = threadIdx.x;
    const unsigned gid = blockIdx.x * 256u + tid, gstride = gridDim.x * 256u;
    float w[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) w[k] = a.weights[k];
    const float Bf = (float)a.B;
    if (a.f_te && (a.g_te || a.gf_te)) {                             // d l_text: -c sign(d) at (y, x) of T, +c sign(d) at (y, Wt-1-x) of Tf
        const float c = w[0] / (Bf * (float)(3 * a.Ht * a.Wt));
        const unsigned rows = (unsigned)a.B * 3u * a.Ht;
        if (dis_wide(a.Wt, ((size_t)a.te) | ((size_t)a.f_te) | ((size_t)a.g_te) | ((size_t)a.gf_te))) {
            const float4* t4 = (const float4*)a.te; const float4* f4 = (const float4*)a.f_te;
            const unsigned wq = (unsigned)a.Wt >> 2, n4 = rows * wq;
            for (unsigned i = gid; i < n4; i += gstride) {
                const unsigned r = i / wq, m = r * wq + (wq - 1 - (i - r * wq));
                const float4 t = t4[i], f = f4[m];
                const float s0 = c * dis_sign(f.w - t.x), s1 = c * dis_sign(f.z - t.y), s2 = c * dis_sign(f.y - t.z), s3 = c * dis_sign(f.x - t.w);
                if (a.g_te) store_once((float4*)a.g_te + i, make_float4(-s0, -s1, -s2, -s3));
                if (a.gf_te) store_once((float4*)a.gf_te + m, make_float4(s3, s2, s1, s0));
            }
        } else {
            const unsigned W = (unsigned)a.Wt, n = rows * W;
            for (unsigned i = gid; i < n; i += gstride) {
                const unsigned r = i / W, m = r * W + (W - 1 - (i - r * W));
                const float s = c * dis_sign(a.f_te[m] - a.te[i]);
                if (a.g_te) a.g_te[i] = -s;
                if (a.gf_te) a.gf_te[m] = s;
            }
        }
    }
    // the norm terms: w / B * diff / norm, exactly 0 for a sample whose norm is 0 (torch.norm's subgradient)
    const unsigned nv = (unsigned)a.B * a.V * 3u, n3 = (unsigned)a.V * 3u;
    if (a.f_ve && (a.g_ve || a.gf_ve)) {
        const float c = w[1] / Bf;
        for (unsigned i = gid; i < nv; i += gstride) {
            const bool isx = i % 3u == 0;
            const float v = a.ve[i], nrm = a.norm[(i / n3) * 2];
            const float d = a.f_ve[i] - (isx ? -v : v);
            const float g = nrm > 0.f ? c * (d / nrm) : 0.f;
            if (a.gf_ve) a.gf_ve[i] = g;
            if (a.g_ve) a.g_ve[i] = isx ? g : -g;
        }
    }
    if (a.j_dv && (a.g_dv || a.gj_dv)) {
        const float c = w[6] / Bf;
        for (unsigned i = gid; i < nv; i += gstride) {
            const float nrm = a.norm[(i / n3) * 2 + 1];
            const float d = a.j_dv[i] - a.dv[i];
            const float g = nrm > 0.f ? c * (d / nrm) : 0.f;
            if (a.gj_dv) a.gj_dv[i] = g;
            if (a.g_dv) a.g_dv[i] = -g;
        }
    }
    if (blockIdx.x != 0 || !a.j_dv) return;
    for (int i = tid; i < a.B; i += 256) {
        // angle2xy: d/d angle[deg] of (cos - cos_t)^2 + (sin - sin_t)^2, for the jitter set (p) and for Ae (t)
        const float ca = w[2] / (Bf * 2.f), ce = w[3] / (Bf * 2.f);
        const float pa = a.j_az[i] * MM_DEG2RAD, ta = a.az[i] * MM_DEG2RAD;
        const float dc = 2.f * (cosf(pa) - cosf(ta)), ds = 2.f * (sinf(pa) - sinf(ta));
        if (a.gj_az) a.gj_az[i] = ca * (dc * (-sinf(pa)) + ds * cosf(pa)) * MM_DEG2RAD;
        if (a.g_az) a.g_az[i] = ca * (dc * sinf(ta) - ds * cosf(ta)) * MM_DEG2RAD;
        const float pe = a.j_el[i] * MM_DEG2RAD, te = a.el[i] * MM_DEG2RAD;
        const float ec = 2.f * (cosf(pe) - cosf(te)), es = 2.f * (sinf(pe) - sinf(te));
        if (a.gj_el) a.gj_el[i] = ce * (ec * (-sinf(pe)) + es * cosf(pe)) * MM_DEG2RAD;
        if (a.g_el) a.g_el[i] = ce * (ec * sinf(te) - es * cosf(te)) * MM_DEG2RAD;
        const float gd = (w[4] / Bf) * (2.f * (a.j_di[i] - a.di[i]));
        if (a.gj_di) a.gj_di[i] = gd;
        if (a.g_di) a.g_di[i] = -gd;
    }
    for (int i = tid; i < a.B * 2; i += 256) {
        const float gb = (w[5] / (Bf * 2.f)) * (2.f * (a.j_bi[i] - a.bi[i]));
        if (a.gj_bi) a.gj_bi[i] = gb;
        if (a.g_bi) a.g_bi[i] = -gb;
    }
}

static int dis_blocks(const MMDisentangleDesc* d) {
    const size_t n = (size_t)d->B * 3 * d->Ht * d->Wt;
    size_t b = (n + 256 * 16 - 1) / (256 * 16);                 // ~16 texels per thread
    if (b < 1) b = 1;
    if (b > 1024) b = 1024;
    return (int)b;
}

// workspace: partial (blocks) | cam (4) | sq (B,2) | norm (B,2) | ticket
static size_t dis_off_cam(const MMDisentangleDesc* d) { return align256((size_t)dis_blocks(d) * sizeof(float)); }
static size_t dis_off_sq(const MMDisentangleDesc* d) { return dis_off_cam(d) + 256; }
static size_t dis_off_norm(const MMDisentangleDesc* d) { return dis_off_sq(d) + align256((size_t)d->B * 2 * sizeof(float)); }
static size_t dis_off_ticket(const MMDisentangleDesc* d) { return dis_off_norm(d) + align256((size_t)d->B * 2 * sizeof(float)); }

size_t disentangle_workspace_bytes(const MMDisentangleDesc* d) { return dis_off_ticket(d) + 256; }

static DisArgs dis_args(const MMDisentangleDesc* d) {
    DisArgs a = {};
    a.B = d->B; a.V = d->V; a.Ht = d->Ht; a.Wt = d->Wt;
    a.te = d->textures; a.ve = d->vertices; a.az = d->azimuths; a.el = d->elevations; a.di = d->distances; a.bi = d->biases; a.dv = d->delta_vertices;
    a.f_te = d->flip_textures; a.f_ve = d->flip_vertices;
    a.j_az = d->jitter_azimuths; a.j_el = d->jitter_elevations; a.j_di = d->jitter_distances; a.j_bi = d->jitter_biases; a.j_dv = d->jitter_delta_vertices;
    a.terms = d->terms;
    char* p = (char*)d->workspace;
    a.partial = (float*)p;
    a.cam = (float*)(p + dis_off_cam(d));
    a.sq = (float*)(p + dis_off_sq(d));
    a.norm = (float*)(p + dis_off_norm(d));
    a.ticket = (unsigned*)(p + dis_off_ticket(d));
    return a;
}

int launch_disentangle_fwd(const MMDisentangleDesc* d, hipStream_t s) {
    const DisArgs a = dis_args(d);
    hipLaunchKernelGGL(dis_fwd_kernel, dim3(dis_blocks(d)), dim3(256), 0, s, a);
    return launch_ok("disentangle_fwd");
}

int launch_disentangle_bwd(const MMDisentangleDesc* d, const MMDisentangleGrads* g, hipStream_t s) {
    DisArgs a = dis_args(d);
    a.weights = g->weights;
    a.g_te = g->textures; a.g_ve = g->vertices; a.g_az = g->azimuths; a.g_el = g->elevations; a.g_di = g->distances; a.g_bi = g->biases; a.g_dv = g->delta_vertices;
    a.gf_te = g->flip_textures; a.gf_ve = g->flip_vertices;
    a.gj_az = g->jitter_azimuths; a.gj_el = g->jitter_elevations; a.gj_di = g->jitter_distances; a.gj_bi = g->jitter_biases; a.gj_dv = g->jitter_delta_vertices;
    hipLaunchKernelGGL(dis_bwd_kernel, dim3(dis_blocks(d)), dim3(256), 0, s, a);
    return launch_ok("disentangle_bwd");
}

}  // namespace mm
