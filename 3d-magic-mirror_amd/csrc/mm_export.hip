// mm_export.hip -- float renders to 8-bit pixels on the device, for gfx950: what the reference's evaluation and visualisation code does on
// the host after every render (trainer.py:546-769, test*.py: to_pil_image / make_grid + permute + (image * 255).astype(uint8) / save_image).
//
// The quantiser is the only arithmetic; every step rounds in fp32, nothing is contracted:
//   trunc:   q = fl(x * 255)                 to_pil_image's pic.mul(255).byte(), numpy's (image * 255.0).astype(np.uint8)
//   nearest: q = fl(fl(x * 255) + 0.5)       save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8)
// then NaN -> 0, clamp to [0, 255], convert toward zero.  Outside [0, 1] the reference's cast is undefined; this one saturates.
// `white` first composes a 4-channel pixel over white with its own alpha, x_c <- fl(fl(x_c * m) + fl(1 - m)), m = x_3 (trainer.py:755-757;
// mm_critic.hip's unmask 0).
//
// export_u8_kernel   image mode: n images (C,H,W) -> any of rgb (n,H,W,3), mask (n,H,W), rgba (n,H,W,4) as bytes.  The three outputs are
//                    flat over the n*H*W pixels, so a lane owns 16 consecutive flat pixels: 3 + 1 + 4 whole aligned 16-byte chunks from
//                    one read of each pixel.  A group may span rows and images.  The pixels past the last whole group go byte by byte.
// export_f32_kernel  the same values as fp32 fl(float(q) / 255) in NCHW planes (what to_tensor of the saved file gives); one lane per pixel.
// export_grid_kernel grid mode: (B,N,C,H,W) -> (N,Hg,Wg,3) bytes, frame n = make_grid(x[:, n, :3], nrow, padding, pad_value) in HWC.  A lane
//                    owns one aligned 16-byte chunk of the flat output: bytes [o, o + 16) lie in the six output pixels from o / 3 on, so the
//                    grid position is decoded once per chunk and stepped five times; six pixel loads, 18 bytes packed, shifted by o % 3,
//                    one store.  Bytes before the first and after the last aligned chunk go byte by byte (32 spare work items).
// Pure streams: no LDS, no scratch, no atomics, no workspace; every output byte is written by one lane (bitwise reproducible).  An NHWC pixel
// is one 16-byte load.  VEC = 0 (a base address off a 16-byte boundary) moves 4 bytes per load and one byte per store.  Offsets are 64-bit;
// work items are counted in an int32 (the entry points refuse more).
#include <hip/hip_runtime.h>

#include "mm_device.h"
#include "mm_quant.h"                                         // quant / unquant: shared with mm_composite.hip

#define MM_EXPORT_BLOCK 256
#define MM_EXPORT_GRID 2048                                   // 256 CUs x 8 workgroups (cdna_hip_programming.md, Guideline 11)
#define MM_EXPORT_EDGE 32                                     // work items for the bytes around the aligned chunks: 16 head + 16 tail

namespace mm {

struct ExportArgs {
    const float* x;                                           // image i = b * N + n at i * C * HW (NCHW) or i * 4 * HW (NHWC)
    unsigned char* rgb; unsigned char* mask; unsigned char* rgba;   // image mode (float* for the fp32 variant)
    unsigned char* grid;
    long long HW, P;                                          // pixels of one image, of all images
    int C, nearest, white;
    int items;                                                // u8: groups of 16 pixels (the last may be partial); grid: chunks + MM_EXPORT_EDGE
    // grid mode
    int B, N, W, xmaps, pad, cellH, cellW, Hg, Wg, head, tail;
    float pad_value;
    long long nchunk;
};

__device__ inline float4 over_white(float4 v) {
    MM_FP_EXACT
    const float w = 1.0f - v.w;
    return make_float4(v.x * v.w + w, v.y * v.w + w, v.z * v.w + w, v.w);
}

// pixel p of image i as (c0, c1, c2, c3); c3 = 0 for C = 3
template <int NHWC, bool VEC>
__device__ inline float4 load_pixel(const float* __restrict__ x, int C, long long HW, long long i, long long p) {
    if constexpr (NHWC) {
        const float* q = x + (i * HW + p) * 4;
        if constexpr (VEC) return *(const float4*)q;
        else return make_float4(q[0], q[1], q[2], q[3]);
    } else {
        const float* q = x + i * C * HW + p;
        return make_float4(q[0], q[HW], q[2 * HW], C == 4 ? q[3 * HW] : 0.0f);
    }
}

// the four bytes of a pixel, byte c in bits [8c, 8c + 8)
__device__ inline unsigned quant_pixel(float4 v, int nearest, int white) {
    if (white) v = over_white(v);
    return quant(v.x, nearest) | (quant(v.y, nearest) << 8) | (quant(v.z, nearest) << 16) | (quant(v.w, nearest) << 24);
}

// ---- image mode, bytes ------------------------------------------------------------------------------------------------------------
template <int NHWC, bool VEC>
__global__ __launch_bounds__(MM_EXPORT_BLOCK) void export_u8_kernel(ExportArgs a) {
    const long long HW = a.HW;
    for (long long g = (long long)blockIdx.x * MM_EXPORT_BLOCK + threadIdx.x; g < a.items; g += (long long)gridDim.x * MM_EXPORT_BLOCK) {
        const long long P0 = g * 16;
        if (VEC && P0 + 16 <= a.P) {
            float4 v[16];
            if constexpr (NHWC) {
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = *(const float4*)(a.x + (P0 + j) * 4);
            } else {
                long long i = P0 / HW, p = P0 - i * HW;
                if ((HW & 15) == 0) {                         // the group lies in one image, 64-byte aligned in each plane
                    const float* q = a.x + i * a.C * HW + p;
                    float4 pl[4][4];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            pl[c][k] = (c < 3 || a.C == 4) ? *(const float4*)(q + c * HW + 4 * k) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v[4 * k] = make_float4(pl[0][k].x, pl[1][k].x, pl[2][k].x, pl[3][k].x);
                        v[4 * k + 1] = make_float4(pl[0][k].y, pl[1][k].y, pl[2][k].y, pl[3][k].y);
                        v[4 * k + 2] = make_float4(pl[0][k].z, pl[1][k].z, pl[2][k].z, pl[3][k].z);
                        v[4 * k + 3] = make_float4(pl[0][k].w, pl[1][k].w, pl[2][k].w, pl[3][k].w);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        v[j] = load_pixel<0, VEC>(a.x, a.C, HW, i, p);
                        if (++p == HW) { p = 0; ++i; }
                    }
                }
            }
            unsigned q[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) q[j] = quant_pixel(v[j], a.nearest, a.white);
            if (a.rgba) {
#pragma unroll
                for (int k = 0; k < 4; ++k) *(uint4*)(a.rgba + P0 * 4 + 16 * k) = make_uint4(q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3]);
            }
            if (a.mask) {
                unsigned m[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    m[k] = (q[4 * k] >> 24) | ((q[4 * k + 1] >> 24) << 8) | ((q[4 * k + 2] >> 24) << 16) | ((q[4 * k + 3] >> 24) << 24);
                *(uint4*)(a.mask + P0) = make_uint4(m[0], m[1], m[2], m[3]);
            }
            if (a.rgb) {
                // four pixels are three words: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
                unsigned w[12];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned p0 = q[4 * k] & 0xffffffu, p1 = q[4 * k + 1] & 0xffffffu, p2 = q[4 * k + 2] & 0xffffffu, p3 = q[4 * k + 3] & 0xffffffu;
                    w[3 * k] = p0 | (p1 << 24);
                    w[3 * k + 1] = (p1 >> 8) | (p2 << 16);
                    w[3 * k + 2] = (p2 >> 16) | (p3 << 8);
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) *(uint4*)(a.rgb + P0 * 3 + 16 * k) = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
            }
        } else {                                              // the pixels past the last whole group (every pixel for VEC = 0)
            const long long P1 = P0 + 16 < a.P ? P0 + 16 : a.P;
            for (long long P = P0; P < P1; ++P) {
                const long long i = NHWC ? 0 : P / HW;
                const unsigned q = quant_pixel(load_pixel<NHWC, VEC>(a.x, a.C, HW, i, P - i * HW), a.nearest, a.white);
                if (a.rgb) { a.rgb[P * 3] = q; a.rgb[P * 3 + 1] = q >> 8; a.rgb[P * 3 + 2] = q >> 16; }
                if (a.mask) a.mask[P] = q >> 24;
                if (a.rgba) { a.rgba[P * 4] = q; a.rgba[P * 4 + 1] = q >> 8; a.rgba[P * 4 + 2] = q >> 16; a.rgba[P * 4 + 3] = q >> 24; }
            }
        }
    }
}

// ---- image mode, fp32 planes ------------------------------------------------------------------------------------------------------
template <int NHWC, bool VEC>
__global__ __launch_bounds__(MM_EXPORT_BLOCK) void export_f32_kernel(ExportArgs a) {
    const long long HW = a.HW;
    float* rgb = (float*)a.rgb; float* mask = (float*)a.mask; float* rgba = (float*)a.rgba;
    for (long long P = (long long)blockIdx.x * MM_EXPORT_BLOCK + threadIdx.x; P < a.P; P += (long long)gridDim.x * MM_EXPORT_BLOCK) {
        const long long i = P / HW, p = P - i * HW;
        const unsigned q = quant_pixel(load_pixel<NHWC, VEC>(a.x, a.C, HW, i, p), a.nearest, a.white);
        const float r = unquant(q & 255u), g = unquant((q >> 8) & 255u), b = unquant((q >> 16) & 255u), m = unquant(q >> 24);
        if (rgb) { float* o = rgb + i * 3 * HW + p; o[0] = r; o[HW] = g; o[2 * HW] = b; }
        if (mask) mask[P] = m;
        if (rgba) { float* o = rgba + i * 4 * HW + p; o[0] = r; o[HW] = g; o[2 * HW] = b; o[3 * HW] = m; }
    }
}

// ---- grid mode --------------------------------------------------------------------------------------------------------------------
// where an output pixel of the sheets lies: frame n, cell row y and line ty of it, cell column xc and column tx of it (lines and columns
// below `pad` are the gutter), and the sheet's line r and column c
struct GridPos { int n, r, c, y, ty, xc, tx; };

__device__ inline GridPos grid_decode(const ExportArgs& a, long long pix) {
    GridPos g;
    const long long per = (long long)a.Hg * a.Wg;
    g.n = (int)(pix / per);
    const long long rem = pix - g.n * per;
    g.r = (int)(rem / a.Wg); g.c = (int)(rem - (long long)g.r * a.Wg);
    g.y = g.r / a.cellH; g.ty = g.r - g.y * a.cellH;
    g.xc = g.c / a.cellW; g.tx = g.c - g.xc * a.cellW;
    return g;
}

__device__ inline void grid_step(const ExportArgs& a, GridPos& g) {
    ++g.c;
    if (++g.tx == a.cellW) { g.tx = 0; ++g.xc; }
    if (g.c == a.Wg) {
        g.c = g.tx = g.xc = 0;
        ++g.r;
        if (++g.ty == a.cellH) { g.ty = 0; ++g.y; }
        if (g.r == a.Hg) { g.r = g.ty = g.y = 0; ++g.n; }
    }
}

// the source of the output pixel: (image, pixel) of the input, and whether there is one: in the gutters and the empty cells pixel 0 of
// image 0 is loaded and dropped.  The last frame's last chunk steps to frame N: nothing uses that position.
__device__ inline bool grid_source(const ExportArgs& a, const GridPos& g, long long& img, long long& p) {
    const long long k = (long long)g.y * a.xmaps + g.xc;
    const bool in = g.ty >= a.pad && g.tx >= a.pad && g.xc < a.xmaps && k < a.B && g.n < a.N;
    img = in ? k * a.N + g.n : 0;
    p = in ? (long long)(g.ty - a.pad) * a.W + (g.tx - a.pad) : 0;
    return in;
}

template <int NHWC, bool VEC>
__global__ __launch_bounds__(MM_EXPORT_BLOCK) void export_grid_kernel(ExportArgs a) {
    const unsigned padq = quant(a.pad_value, a.nearest) * 0x010101u;
    for (long long item = (long long)blockIdx.x * MM_EXPORT_BLOCK + threadIdx.x; item < a.items; item += (long long)gridDim.x * MM_EXPORT_BLOCK) {
        if (item < a.nchunk) {
            const long long o = a.head + item * 16;
            const long long pix = o / 3;
            const int ch = (int)(o - pix * 3);
            GridPos g = grid_decode(a, pix);
            float4 v[6];
            bool in[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                long long img, p;
                in[j] = grid_source(a, g, img, p);
                v[j] = load_pixel<NHWC, VEC>(a.x, a.C, a.HW, img, p);
                grid_step(a, g);
            }
            unsigned q[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) q[j] = in[j] ? quant_pixel(v[j], a.nearest, a.white) & 0xffffffu : padq;
            // 18 bytes in five words, then the 16 from byte `ch` on
            unsigned w[5];
            w[0] = q[0] | (q[1] << 24); w[1] = (q[1] >> 8) | (q[2] << 16); w[2] = (q[2] >> 16) | (q[3] << 8);
            w[3] = q[4] | (q[5] << 24); w[4] = q[5] >> 8;
            const int sh = ch * 8;
            unsigned r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = (unsigned)((((unsigned long long)w[k + 1] << 32) | w[k]) >> sh);
            *(uint4*)(a.grid + o) = make_uint4(r[0], r[1], r[2], r[3]);
        } else {
            const int e = (int)(item - a.nchunk);              // [0, 16): head byte e; [16, 32): tail byte e - 16
            long long o;
            if (e < 16) { if (e >= a.head) continue; o = e; }
            else { if (e - 16 >= a.tail) continue; o = a.head + a.nchunk * 16 + (e - 16); }
            const long long pix = o / 3;
            const int ch = (int)(o - pix * 3);
            const GridPos g = grid_decode(a, pix);
            long long img, p;
            const bool in = grid_source(a, g, img, p);
            const unsigned q = in ? quant_pixel(load_pixel<NHWC, VEC>(a.x, a.C, a.HW, img, p), a.nearest, a.white) : padq;
            a.grid[o] = q >> (8 * ch);
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static dim3 export_grid_dim(long long lanes) {
    const long long wg = (lanes + MM_EXPORT_BLOCK - 1) / MM_EXPORT_BLOCK;
    return dim3((unsigned)(wg < MM_EXPORT_GRID ? wg : MM_EXPORT_GRID));
}

// the sheet of grid mode: make_grid's arithmetic.  One image is the sheet itself, without gutters.
void export_grid_geometry(const MMExportDesc* d, long long* xmaps, long long* pad, long long* Hg, long long* Wg) {
    if (d->B == 1) { *xmaps = 1; *pad = 0; *Hg = d->H; *Wg = d->W; return; }
    *xmaps = d->nrow < d->B ? d->nrow : d->B;
    const long long ymaps = (d->B + *xmaps - 1) / *xmaps;
    *pad = d->padding;
    *Hg = ((long long)d->H + d->padding) * ymaps + d->padding;
    *Wg = ((long long)d->W + d->padding) * *xmaps + d->padding;
}

#define MM_EXPORT_LAUNCH(kernel, nhwc, vec, grid, s, a)                                                              \
    do {                                                                                                             \
        if (nhwc) { if (vec) hipLaunchKernelGGL((kernel<1, true>), grid, dim3(MM_EXPORT_BLOCK), 0, s, a);            \
                    else hipLaunchKernelGGL((kernel<1, false>), grid, dim3(MM_EXPORT_BLOCK), 0, s, a); }             \
        else { if (vec) hipLaunchKernelGGL((kernel<0, true>), grid, dim3(MM_EXPORT_BLOCK), 0, s, a);                 \
               else hipLaunchKernelGGL((kernel<0, false>), grid, dim3(MM_EXPORT_BLOCK), 0, s, a); }                  \
    } while (0)

int launch_export_images(const MMExportDesc* d, hipStream_t s) {
    ExportArgs a = {};
    a.x = d->x; a.rgb = (unsigned char*)d->out_rgb; a.mask = (unsigned char*)d->out_mask; a.rgba = (unsigned char*)d->out_rgba;
    a.C = d->C; a.nearest = d->rounding; a.white = d->white != 0;
    a.HW = (long long)d->H * d->W; a.P = (long long)d->B * d->N * a.HW;
    const int nhwc = d->nhwc != 0;
    const bool vec = aligned16(a.x) && aligned16(a.rgb) && aligned16(a.mask) && aligned16(a.rgba);
    if (d->as_float) {
        MM_EXPORT_LAUNCH(export_f32_kernel, nhwc, vec, export_grid_dim(a.P), s, a);
        return launch_ok("export_f32");
    }
    a.items = (int)((a.P + 15) / 16);
    MM_EXPORT_LAUNCH(export_u8_kernel, nhwc, vec, export_grid_dim(a.items), s, a);
    return launch_ok("export_u8");
}

int launch_export_grid(const MMExportDesc* d, hipStream_t s) {
    ExportArgs a = {};
    long long xmaps, pad, Hg, Wg;
    export_grid_geometry(d, &xmaps, &pad, &Hg, &Wg);
    a.x = d->x; a.grid = d->out_grid;
    a.C = d->C; a.nearest = d->rounding; a.white = d->white != 0; a.pad_value = d->pad_value;
    a.HW = (long long)d->H * d->W;
    a.B = d->B; a.N = d->N; a.W = d->W; a.xmaps = (int)xmaps; a.pad = (int)pad;
    a.cellH = (int)(d->H + pad); a.cellW = (int)(d->W + pad); a.Hg = (int)Hg; a.Wg = (int)Wg;
    const long long total = (long long)d->N * Hg * Wg * 3;
    long long head = (16 - (long long)((uintptr_t)a.grid & 15)) & 15;
    if (head > total) head = total;
    a.head = (int)head; a.nchunk = (total - head) / 16; a.tail = (int)(total - head - a.nchunk * 16);
    a.items = (int)(a.nchunk + MM_EXPORT_EDGE);
    MM_EXPORT_LAUNCH(export_grid_kernel, d->nhwc != 0, aligned16(a.x), export_grid_dim(a.items), s, a);
    return launch_ok("export_grid");
}

}  // namespace mm
