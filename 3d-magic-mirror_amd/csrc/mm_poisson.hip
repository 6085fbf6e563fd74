// mm_poisson.hip -- renders blended into backgrounds by Poisson (seamless-cloning) editing, as 8-bit frames, for gfx950: the system the
// reference's poisson_image_editing.py:33-108 builds with offset (0,0) and hands to one sparse direct solve per frame and channel on the
// host, solved here by a fixed number of red-black SOR sweeps, one launch per batch of frames.
//
// Per frame o and colour channel c, every step in fp32, rounded as written, no contraction:
//   s         channel c of render fg_index[o] (the source), untouched
//   t         channel c of background bg_index[o] behind the reflection pad, resized to (H,W) by the host's tap tables, x first, then y,
//             sums in ascending tap index from 0, NO blur: bit for bit mm_pyramid.hip's level 0 of the background (mm_frame.h's pieces)
//   in        mask[fg_index[o]][y][x] != 0 where a mask is given, otherwise quant(alpha, trunc) != 0 on the render's channel 3: the byte
//             mm_export_images would store, then the reference's mask[mask != 0] = 1
//   pinned    border 0 ("reference"): cells outside the mask that are not on the image's outer row or column (the reference's
//             range(1, n - 1) loops); border 1 ("pinned"): every cell outside the mask.  x = t, never touched.
//   free      all other cells: 4 x_p - sum x_q = b_p over the 4-neighbours q inside the image.  Inside the mask
//             b = fl(fl(4 s) - fl(fl(sl + sr) + fl(su + sd))), a neighbour outside the image being 0; outside the mask (the outer-border
//             cells of "reference") b = t.
//   solve     x = t everywhere; `sweeps` times: the free cells with (y + x) even, then those with (y + x) odd, each
//             x <- fl(x + fl(omega * fl(fl(fl(b + fl(fl(l + r) + fl(u + d))) * 0.25) - x))), a neighbour outside the image read as 0.
//             Cells of one colour do not read each other, so the result does not depend on which lane has which cell.  No convergence
//             test, no early exit.
//   quantise  mm_export.hip's quantiser (mm_quant.h): the solution leaves [0, 1]; it saturates and sends NaN to 0.
//
// One workgroup of MM_POISSON_BLOCK solves one (frame, channel) plane, which stays in LDS from the first sweep to the last: no memory
// traffic between sweeps, no atomics, no scratch, two barriers per sweep.  The plane has a ring of zeros, so a sweep has no edge branches,
// and is stored as TWO COMPACTED COLOUR PLANES: padded cell (py, px) = (y + 1, x + 1) of colour (py + px) & 1 lies at [py * S + (px >> 1)]
// of its colour's plane, S = (W + 3) / 2.  A lane that walks along a row of one colour then reads consecutive words of the other plane for
// each of its four neighbours -- left (px - 1) >> 1 = j - 1 + p, right j + p, with p = px & 1 the same for the whole row, up and down j of
// the rows above and below -- where a stride-2 walk over a row-major plane would put two lanes on every bank.  A lane owns slots
// i = S + tid + n * MM_POISSON_BLOCK, n < NPL, of EACH colour plane (the linear index is the LDS address: no division inside a sweep) and
// keeps their x and b in registers and, one bit per slot, whether the slot is a free cell and the row's p; only free cells ever execute
// an update, so neither the ring, the dummy slot that an odd width leaves at a row's end, nor a pinned cell is written after the set-up.
// NPL is a template parameter (register arrays, fully unrolled); the host picks the smallest instance that covers H * S slots.  The largest
// instance keeps only b in registers and reads its own x from LDS (XREG below).
// Dynamic LDS only: 4 * (2 * plane + stage) bytes, plane = (H + 2) * S and stage = W times the most source rows the vertical resize of a
// band of MM_FRAME_ROWS output rows reads, each rounded up to 4 floats.  A call that needs more than 160 KiB is refused.
#include <hip/hip_runtime.h>

#include "mm_frame.h"

#ifndef MM_POISSON_BLOCK
#define MM_POISSON_BLOCK 1024                                 // profiles/poisson_kernels.md has what 256 and 512 measured
#endif
#define MM_PW MM_FRAME_ROW_WORDS

namespace mm {

struct PoiArgs {
    const float* fg; const float* bg; const unsigned char* mask; const int* par; void* out;
    int B, H, W, n_fg, n_bg, bgC, nhwc, pl, pr, pt, pb, nearest, as_float, pinned, sweeps;
    float omega;
    int S;                                                    // words in a row of a colour plane
    int plane;                                                // floats in a colour plane
    int stage;                                                // floats in the resize's staging rows
};

// where the tables lie in MMPoissonDesc.params (32-bit words)
struct PoiLayout { long long fg_index, bg_index, bg_y, bg_x, words; };
__host__ __device__ inline PoiLayout poisson_layout(int B, int H, int W) {
    PoiLayout l;
    l.fg_index = 0; l.bg_index = B;
    l.bg_y = 2LL * B; l.bg_x = l.bg_y + (long long)MM_PW * H;
    l.words = l.bg_x + (long long)MM_PW * W;
    return l;
}

// XREG: the lane keeps its cells' x in registers too (four LDS reads per update, not five); the largest instance does not, to stay
// inside the 128 registers that 1024 lanes leave each other
template <int NPL, bool XREG>
__global__ __launch_bounds__(MM_POISSON_BLOCK) void poisson_kernel(PoiArgs a) {
    MM_FP_EXACT
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* P0 = (float*)smem;                                 // the cells with (py + px) even
    float* P1 = P0 + a.plane;                                 // ... odd
    float* T = P1 + a.plane;

    const int tid = threadIdx.x, H = a.H, W = a.W, S = a.S;
    const int o = blockIdx.x / 3, c = blockIdx.x - 3 * o;
    const PoiLayout l = poisson_layout(a.B, H, W);
    const long long fi = frame_index(a.par + l.fg_index, o, a.n_fg), bi = frame_index(a.par + l.bg_index, o, a.n_bg);
    const long long HW = (long long)H * W;
    const FrameFg fg_at = {a.fg + fi * 4 * HW, HW, W, a.nhwc};
    const int Hp = H + a.pt + a.pb, Wp = W + a.pl + a.pr, pl = a.pl;
    const int* ty = a.par + l.bg_y;
    const int* tx = a.par + l.bg_x;

    for (int i = tid; i < 2 * a.plane; i += MM_POISSON_BLOCK) P0[i] = 0.0f;       // the ring, and the dummy slots of an odd width
    __syncthreads();

    // the target, band by band as the siblings make it: horizontal resize of the padded rows straight from memory, then the vertical one
    const float* bgp = a.bg + (bi * a.bgC + c) * HW;
    for (int y0 = 0; y0 < H; y0 += MM_FRAME_ROWS) {
        const int y1 = min(y0 + MM_FRAME_ROWS, H);
        int c_lo, nsrc;
        frame_src_rows(ty, y0, y1, 0, Hp, c_lo, nsrc);
        if ((long long)nsrc * W > a.stage) return;            // (uniform) a device table that is not the one the host sized the LDS from
        for (int i = tid; i < nsrc * W; i += MM_POISSON_BLOCK) {
            const int row = i / W, x = i - row * W;
            const float* s = bgp + (long long)reflecti(c_lo + row - a.pt, H) * W;
            T[i] = frame_resize_sum(tx, x, 0, [=](int j) { return s[reflecti(clampi(j, 0, Wp - 1) - pl, W)]; });
        }
        __syncthreads();
        for (int i = tid; i < (y1 - y0) * W; i += MM_POISSON_BLOCK) {
            const int row = i / W, x = i - row * W, y = y0 + row;
            const float acc = frame_resize_sum(ty, y, 0, [=](int j) { return T[clampi(clampi(j, 0, Hp - 1) - c_lo, 0, nsrc - 1) * W + x]; });
            const int py = y + 1, px = x + 1;
            (((py + px) & 1) ? P1 : P0)[py * S + (px >> 1)] = acc;
        }
        __syncthreads();
    }

    // the lane's cells: x and b in registers, one bit per slot for "a free cell" and for the row's p
    float xr[2][XREG ? NPL : 1], br[2][NPL];
    unsigned long long fr[2] = {0ULL, 0ULL}, pa[2] = {0ULL, 0ULL};
    const int end = (H + 1) * S;                              // slots [S, end) are rows py = 1 .. H
    const int qb = MM_POISSON_BLOCK / S, rb = MM_POISSON_BLOCK - qb * S;
    int py = (S + tid) / S, j = S + tid - py * S;             // slot n = 0; slot n + 1 lies MM_POISSON_BLOCK = qb * S + rb words on
#pragma unroll
    for (int n = 0; n < NPL; ++n) {
        const int i = S + tid + n * MM_POISSON_BLOCK;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            if (XREG) xr[cc][n] = 0.0f;
            br[cc][n] = 0.0f;
            const int p = (py + cc) & 1, px = 2 * j + p;
            pa[cc] |= (unsigned long long)p << n;
            if (i >= end || px < 1 || px > W) continue;       // beyond the last row, the ring, or the dummy slot
            const int y = py - 1, x = px - 1;
            const bool inside = a.mask ? a.mask[(fi * H + y) * W + x] != 0 : quant(fg_at(3, y, x), 0) != 0u;
            const bool edge = y == 0 || y == H - 1 || x == 0 || x == W - 1;
            if (!inside && (a.pinned || !edge)) continue;     // pinned: it keeps t
            fr[cc] |= 1ULL << n;
            const float t = (cc ? P1 : P0)[i];
            if (XREG) xr[cc][n] = t;
            if (inside) {
                const float s = fg_at(c, y, x);
                const float sl = x > 0 ? fg_at(c, y, x - 1) : 0.0f, sr = x < W - 1 ? fg_at(c, y, x + 1) : 0.0f;
                const float su = y > 0 ? fg_at(c, y - 1, x) : 0.0f, sd = y < H - 1 ? fg_at(c, y + 1, x) : 0.0f;
                br[cc][n] = 4.0f * s - ((sl + sr) + (su + sd));
            } else {
                br[cc][n] = t;
            }
        }
        py += qb; j += rb;
        if (j >= S) { j -= S; ++py; }
    }
    // (every lane read its own slots only, and the target's last barrier lies before: the sweeps may start)

    const float om = a.omega;
    for (int sweep = 0; sweep < a.sweeps; ++sweep) {
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            float* own = cc ? P1 : P0;
            const float* oth = cc ? P0 : P1;
#pragma unroll
            for (int n = 0; n < NPL; ++n) {
                if (!((fr[cc] >> n) & 1ULL)) continue;
                const int i = S + tid + n * MM_POISSON_BLOCK, p = (int)((pa[cc] >> n) & 1ULL);
                const float lf = oth[i - 1 + p], rt = oth[i + p], up = oth[i - S], dn = oth[i + S];
                float x = XREG ? xr[cc][n] : own[i];
                x = x + om * (((br[cc][n] + ((lf + rt) + (up + dn))) * 0.25f) - x);
                if (XREG) xr[cc][n] = x;
                own[i] = x;
            }
            __syncthreads();
        }
    }

    // every cell's value is in LDS behind a barrier (the last sweep's, or the target's): the quantiser, one lane per output value
    unsigned char* outb = (unsigned char*)a.out;
    float* outf = (float*)a.out;
    for (int i = tid; i < H * W; i += MM_POISSON_BLOCK) {
        const int y = i / W, x = i - y * W, py = y + 1, px = x + 1;
        const unsigned q = quant((((py + px) & 1) ? P1 : P0)[py * S + (px >> 1)], a.nearest);
        if (a.as_float) outf[((long long)o * 3 + c) * HW + i] = unquant(q);
        else outb[((long long)o * HW + i) * 3 + c] = (unsigned char)q;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// the bytes of LDS a call needs, from the host's copy of the tables: the two colour planes and the staging rows of the tallest band.
// Fills the carving of `a`.
long long poisson_lds_bytes(const MMPoissonDesc* d, PoiArgs* a) {
    const PoiLayout l = poisson_layout(d->B, d->H, d->W);
    const int Hp = d->H + d->bg_pad[2] + d->bg_pad[3];
    long long rows = 0;
    for (int y0 = 0; y0 < d->H; y0 += MM_FRAME_ROWS) {
        const int y1 = y0 + MM_FRAME_ROWS < d->H ? y0 + MM_FRAME_ROWS : d->H;
        int c_lo, n;
        frame_src_rows(d->params_host + l.bg_y, y0, y1, 0, Hp, c_lo, n);
        rows = n > rows ? n : rows;
    }
    const long long S = ((long long)d->W + 3) / 2;
    const long long plane = (((long long)d->H + 2) * S + 3) & ~3LL;
    const long long stage = (rows * d->W + 3) & ~3LL;
    const long long lim = 0x7fffffff;
    if (a) { a->S = (int)S; a->plane = plane < lim ? (int)plane : (int)lim; a->stage = stage < lim ? (int)stage : (int)lim; }
    return 4 * (2 * plane + stage);
}

int launch_poisson(const MMPoissonDesc* d, hipStream_t s) {
    PoiArgs a = {};
    a.fg = d->renders; a.bg = d->backgrounds; a.mask = d->mask; a.par = d->params; a.out = d->out;
    a.B = d->B; a.H = d->H; a.W = d->W; a.n_fg = d->n_fg; a.n_bg = d->n_bg; a.bgC = d->bg_C; a.nhwc = d->fg_nhwc != 0;
    a.pl = d->bg_pad[0]; a.pr = d->bg_pad[1]; a.pt = d->bg_pad[2]; a.pb = d->bg_pad[3];
    a.nearest = d->rounding; a.as_float = d->as_float != 0; a.pinned = d->border != 0; a.sweeps = d->sweeps; a.omega = d->omega;
    const long long lds = poisson_lds_bytes(d, &a);
    // slots per lane and colour: the rows py = 1 .. H of a colour plane over the workgroup.  Two planes within 160 KiB are 20 480 slots
    // each at most, so with 1024 lanes the largest instance covers every call that passed the LDS check
    const long long need = ((long long)d->H * a.S + MM_POISSON_BLOCK - 1) / MM_POISSON_BLOCK;
    void (*kernel)(PoiArgs) = nullptr;
    if (need <= 1) kernel = poisson_kernel<1, true>;
    else if (need <= 2) kernel = poisson_kernel<2, true>;
    else if (need <= 3) kernel = poisson_kernel<3, true>;
    else if (need <= 5) kernel = poisson_kernel<5, true>;           // 128 x 64
    else if (need <= 9) kernel = poisson_kernel<9, true>;           // 128 x 128
    else if (need <= 14) kernel = poisson_kernel<14, true>;
    else if (need <= 20) kernel = poisson_kernel<20, false>;
#if MM_POISSON_BLOCK <= 512                                   // (a measurement build with a smaller workgroup: more slots per lane)
    else if (need <= 34) kernel = poisson_kernel<34, true>;
#endif
    if (!kernel) return MM_ERR_UNSUPPORTED;
    if (allow_large_lds((const void*)kernel, lds, MM_FRAME_LDS, "poisson_lds") != MM_OK) return MM_ERR_LAUNCH;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(d->B * 3)), dim3(MM_POISSON_BLOCK), (size_t)lds, s, a);
    return launch_ok("poisson");
}

}  // namespace mm
