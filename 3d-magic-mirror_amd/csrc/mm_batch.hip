// mm_batch.hip -- training batches assembled from device-resident 8-bit images, for gfx950: what the reference's DataLoader workers do per
// sample in Pillow (datasets/bird.py:69-136, datasets/market.py:77-145: flip, expand, crop, pad to square, bicubic resize, nearest resize of the
// mask, threshold, to_tensor, composite over white), one launch per batch.  The mirror of mm_export.hip: bytes in, floats out.
//
// The kernel knows only the canonical record (include/mm_render.h, MMBatchDesc): a window of the (mirrored) source, clipped, resized to
// (Wr,Hr), shifted, mirrored, divided by 255 and composed.  The resize is Pillow's, to the bit:
//   per axis and output index xx, in fp64:  scale = in / out, fs = max(scale, 1), support = 2 fs, c = (xx + 0.5) scale,
//     taps [max(0, (int)(c - support + 0.5)), min(in, (int)(c + support + 0.5))), w = cubic((x - c + 0.5) * (1 / fs)), a = -0.5,
//     normalised by their sum added in index order, k = (int)(w 2^22 -+ 0.5);  byte = clamp((2^21 + sum k p) >> 22, 0, 255) in int32.
//   The horizontal pass runs first, to clamped BYTES; the vertical pass runs on those bytes (the clamp between them is visible).
//   The mask is Pillow's nearest -- index (int)xo, xo = a / 2 stepped by a = in / out in fp64, an index past the end leaves 0 --, then > 160.
// Only + - * / in fp64 and integer arithmetic, compiled without contraction; the last step is one correctly rounded fp32 divide.
//
// One workgroup of 256 per (sample, tile of MM_BATCH_ROWS output rows):
//   1. tables in LDS: the horizontal taps of all Wr columns (lane per column, taps in index order), the vertical taps of the tile's rows
//      (the eight highest lanes), both nearest tables.
//   2. horizontal pass over just the canvas rows the tile's vertical taps read, into LDS as bytes (rows x Wr x 3).  A lane owns one
//      (row, column) and walks its taps along x; neighbouring lanes read neighbouring source bytes (scale * 3 bytes apart), at whatever byte
//      alignment the image has in the pool.  Adjacent tiles recompute 2 * support rows of overlap.
//   3. vertical pass from LDS, mask, shift, flip, divide, composite; the four planes are written with x along the lanes.
// LDS is dynamic, carved for the largest sample of the batch (batch_lds_bytes); a canvas / resized ratio above MM_BATCH_MAX_RATIO = 16 on
// either axis, or tables beyond 160 KiB, are refused by the entry point.  No workspace, no atomics, no scratch; every output is written by one lane.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mm_device.h"

#define MM_BATCH_BLOCK 256
#define MM_BATCH_LDS (160 * 1024)

namespace mm {

struct BatchArgs {
    const unsigned char* images; const unsigned char* segs;
    const long long* offsets; const int* sizes; const int* rec;
    float* out;
    int H, W, bg, n_images;
    int ksx, ksy, rows, wr;                                   // LDS carving: tap-table strides, row-buffer rows, widest resize of the batch
};

__device__ inline double cubic(double t) {
    MM_FP_EXACT
    const double a = -0.5;
    if (t < 0.0) t = -t;
    if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
    if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * a;
    return 0.0;
}

struct Axis { double scale, support, inv; };
__host__ __device__ inline Axis axis_of(int n_in, int n_out) {
    Axis s;
    s.scale = (double)n_in / (double)n_out;
    const double fs = s.scale < 1.0 ? 1.0 : s.scale;
    s.support = 2.0 * fs;
    s.inv = 1.0 / fs;
    return s;
}

// taps [lo, hi) of output index xx
__device__ inline void tap_bounds(const Axis& s, int n_in, int xx, int& lo, int& hi) {
    MM_FP_EXACT
    const double c = ((double)xx + 0.5) * s.scale;
    lo = (int)(c - s.support + 0.5);
    hi = (int)(c + s.support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > n_in) hi = n_in;
}

// the integer weights of output index xx into k[0, hi - lo)
__device__ inline void tap_weights(const Axis& s, int xx, int lo, int hi, int* k) {
    MM_FP_EXACT
    const double c = ((double)xx + 0.5) * s.scale;
    double ww = 0.0;
    for (int x = lo; x < hi; ++x) ww += cubic(((double)x - c + 0.5) * s.inv);
    for (int x = lo; x < hi; ++x) {
        double w = cubic(((double)x - c + 0.5) * s.inv);
        if (ww != 0.0) w = w / ww;
        k[x - lo] = w < 0.0 ? (int)(-0.5 + w * 4194304.0) : (int)(0.5 + w * 4194304.0);
    }
}

// Pillow's nearest index of output index xx, -1 for none: the coordinate is STEPPED, one fp64 addition per index
__device__ inline int nearest_index(int n_in, int n_out, int xx) {
    MM_FP_EXACT
    const double a = (double)n_in / (double)n_out;
    double xo = a * 0.5;
    for (int i = 0; i < xx; ++i) xo += a;
    const int xin = xo < 0.0 ? -1 : (int)xo;
    return xin < n_in ? xin : -1;
}

__device__ inline int clip8(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(MM_BATCH_BLOCK) void assemble_batch_kernel(BatchArgs a) {
    extern __shared__ int lds[];
    int* hk = lds;                                            // [wr][ksx]
    int* vk = hk + a.wr * a.ksx;                              // [MM_BATCH_ROWS][ksy]
    int* hmin = vk + MM_BATCH_ROWS * a.ksy;                   // [wr] first tap, [wr] tap count, [wr] nearest
    int* hn = hmin + a.wr;
    int* nx = hn + a.wr;
    int* vmin = nx + a.wr;                                    // the same for the tile's rows
    int* vn = vmin + MM_BATCH_ROWS;
    int* ny = vn + MM_BATCH_ROWS;
    unsigned char* rowbuf = (unsigned char*)(ny + MM_BATCH_ROWS);   // [rows][Wr][3]

    const int tid = threadIdx.x, b = blockIdx.y, y_first = blockIdx.x * MM_BATCH_ROWS;
    const int* r = a.rec + b * 16;
    const int img = r[0], flip_src = r[1], x0 = r[2], y0 = r[3], Wc = r[4], Hc = r[5];
    const int Wr = r[10], Hr = r[11], dx = r[12], dy = r[13], flip_out = r[14];
    // the entry point checked the host's copy of the records; a device copy that differs gives zeros, never a wild address
    const bool sane = img >= 0 && img < a.n_images && Wc >= 1 && Hc >= 1 && Wr >= 1 && Wr <= a.wr && Hr >= 1;
    const int Hs = sane ? a.sizes[2 * img] : 0, Ws = sane ? a.sizes[2 * img + 1] : 0;
    const long long off = sane ? a.offsets[img] : 0;
    // where the window, the clip rectangle and the image meet, in canvas coordinates
    const int ax0 = max(max(r[6], 0), x0) - x0, ax1 = min(min(r[8], Ws), x0 + Wc) - x0;
    const int ay0 = max(max(r[7], 0), y0) - y0, ay1 = min(min(r[9], Hs), y0 + Hc) - y0;
    // resized rows [rlo, rhi) that this tile's output rows read
    const int y_end = min(y_first + MM_BATCH_ROWS, a.H);
    const int rlo = max(y_first + dy, 0), rhi = sane ? min(y_end + dy, Hr) : 0;
    const bool work = rlo < rhi;                              // uniform over the workgroup
    int ymin_t = 0, nrows = 0;

    if (work) {
        const Axis sx = axis_of(Wc, Wr), sy = axis_of(Hc, Hr);
        for (int xx = tid; xx < Wr; xx += MM_BATCH_BLOCK) {
            int lo, hi;
            tap_bounds(sx, Wc, xx, lo, hi);
            if (hi - lo > a.ksx) hi = lo + a.ksx;             // cannot happen: ksx = 2 ceil(support) + 1
            hmin[xx] = lo; hn[xx] = hi - lo;
            tap_weights(sx, xx, lo, hi, hk + xx * a.ksx);
            nx[xx] = nearest_index(Wc, Wr, xx);
        }
        const int rr = MM_BATCH_BLOCK - 1 - tid;              // the highest lanes: beside the columns' lanes, not behind them
        if (rr < rhi - rlo) {
            int lo, hi;
            tap_bounds(sy, Hc, rlo + rr, lo, hi);
            if (hi - lo > a.ksy) hi = lo + a.ksy;
            vmin[rr] = lo; vn[rr] = hi - lo;
            tap_weights(sy, rlo + rr, lo, hi, vk + rr * a.ksy);
            ny[rr] = nearest_index(Hc, Hr, rlo + rr);
        }
        int lo, hi, ymax_t;
        tap_bounds(sy, Hc, rlo, ymin_t, hi);
        tap_bounds(sy, Hc, rhi - 1, lo, ymax_t);
        nrows = min(ymax_t - ymin_t, a.rows);                 // <= a.rows by batch_rows()'s bound
        __syncthreads();

        // ---- horizontal pass: canvas rows [ymin_t, ymin_t + nrows) to bytes ----
        int row = tid / Wr, xr = tid - row * Wr;
        while (row < nrows) {
            int acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21;
            const int cy = ymin_t + row;
            if (cy >= ay0 && cy < ay1) {
                const int lo = hmin[xr];
                const int jlo = max(0, ax0 - lo), jhi = min(hn[xr], ax1 - lo);
                if (jlo < jhi) {
                    const int mx = x0 + lo + jlo;             // mirrored source x of the first tap
                    const int sxp = flip_src ? Ws - 1 - mx : mx;
                    const int step = flip_src ? -3 : 3;
                    const unsigned char* p = a.images + 3 * (off + (long long)(y0 + cy) * Ws + sxp);
                    const int* k = hk + xr * a.ksx;
                    for (int j = jlo; j < jhi; ++j) {
                        const int kj = k[j];
                        acc0 += kj * (int)p[0]; acc1 += kj * (int)p[1]; acc2 += kj * (int)p[2];
                        p += step;
                    }
                }
            }
            unsigned char* o = rowbuf + (row * Wr + xr) * 3;
            o[0] = (unsigned char)clip8(acc0); o[1] = (unsigned char)clip8(acc1); o[2] = (unsigned char)clip8(acc2);
            xr += MM_BATCH_BLOCK;
            while (xr >= Wr) { xr -= Wr; ++row; }
        }
    }
    __syncthreads();

    // ---- vertical pass, mask, shift, flip, divide, composite ----
    const long long plane = (long long)a.H * a.W;
    int ro = tid / a.W, x = tid - ro * a.W;
    while (y_first + ro < y_end) {
        const int y = y_first + ro;
        const int ry = y + dy, rx = (flip_out ? a.W - 1 - x : x) + dx;
        int q0 = 0, q1 = 0, q2 = 0, m = 0;
        if (work && ry >= rlo && ry < rhi && rx >= 0 && rx < Wr) {
            const int rr = ry - rlo;
            const int* k = vk + rr * a.ksy;
            const unsigned char* p = rowbuf + ((vmin[rr] - ymin_t) * Wr + rx) * 3;
            int acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21;
            const int n = vn[rr];
            for (int j = 0; j < n; ++j) {
                const int kj = k[j];
                acc0 += kj * (int)p[0]; acc1 += kj * (int)p[1]; acc2 += kj * (int)p[2];
                p += Wr * 3;
            }
            q0 = clip8(acc0); q1 = clip8(acc1); q2 = clip8(acc2);
            const int mxc = nx[rx], myc = ny[rr];
            if (mxc >= ax0 && mxc < ax1 && myc >= ay0 && myc < ay1) {
                const int mx = x0 + mxc;
                m = a.segs[off + (long long)(y0 + myc) * Ws + (flip_src ? Ws - 1 - mx : mx)] > 160;
            }
        }
        float v0, v1, v2;
        {
            MM_FP_EXACT
            v0 = (float)q0 / 255.0f; v1 = (float)q1 / 255.0f; v2 = (float)q2 / 255.0f;
        }
        if (!a.bg && !m) v0 = v1 = v2 = 1.0f;
        float* o = a.out + (long long)b * 4 * plane + (long long)y * a.W + x;
        o[0] = v0; o[plane] = v1; o[2 * plane] = v2; o[3 * plane] = m ? 1.0f : 0.0f;
        x += MM_BATCH_BLOCK;
        while (x >= a.W) { x -= a.W; ++ro; }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// taps per output index at most: Pillow's ksize = 2 ceil(support) + 1
int batch_ksize(int n_in, int n_out) {
    const Axis s = axis_of(n_in, n_out);
    int c = (int)s.support;
    if ((double)c < s.support) ++c;
    return 2 * c + 1;
}

// canvas rows the vertical taps of MM_BATCH_ROWS consecutive output rows span at most: the first row's first tap is (int)(c - support + 0.5)
// or later, the last row's last is before (int)(c + (ROWS - 1) scale + support + 0.5), so the span is at most
// floor((ROWS - 1) scale) + ceil(2 support) + 1 <= floor((ROWS - 1) scale) + ksize
int batch_rows(int n_in, int n_out) {
    return (int)((MM_BATCH_ROWS - 1) * axis_of(n_in, n_out).scale) + batch_ksize(n_in, n_out) + 1;
}

// fills the carving of `a` from the host's records; returns the bytes of LDS
long long batch_lds_bytes(const MMBatchDesc* d, BatchArgs* a) {
    int ksx = 0, ksy = 0, rows = 0, wr = 0;
    for (int b = 0; b < d->B; ++b) {
        const int32_t* r = d->records_host + (size_t)b * 16;
        ksx = std::max(ksx, batch_ksize(r[4], r[10]));
        ksy = std::max(ksy, batch_ksize(r[5], r[11]));
        rows = std::max(rows, batch_rows(r[5], r[11]));
        wr = std::max(wr, (int)r[10]);
    }
    if (a) { a->ksx = ksx; a->ksy = ksy; a->rows = rows; a->wr = wr; }
    return 4LL * ((long long)wr * ksx + MM_BATCH_ROWS * ksy + 3LL * wr + 3 * MM_BATCH_ROWS) + ((long long)rows * wr * 3 + 3) / 4 * 4;
}

int launch_assemble_batch(const MMBatchDesc* d, hipStream_t s) {
    BatchArgs a = {};
    a.images = d->images; a.segs = d->segs; a.offsets = (const long long*)d->offsets; a.sizes = d->sizes; a.rec = d->records;
    a.out = d->out; a.H = d->H; a.W = d->W; a.bg = d->bg != 0; a.n_images = d->n_images;
    const long long lds = batch_lds_bytes(d, &a);
    if (allow_large_lds((const void*)assemble_batch_kernel, lds, MM_BATCH_LDS, "assemble_batch_lds") != MM_OK) return MM_ERR_LAUNCH;
    const dim3 grid((unsigned)((d->H + MM_BATCH_ROWS - 1) / MM_BATCH_ROWS), (unsigned)d->B);
    hipLaunchKernelGGL(assemble_batch_kernel, grid, dim3(MM_BATCH_BLOCK), (size_t)lds, s, a);
    return launch_ok("assemble_batch");
}

}  // namespace mm
