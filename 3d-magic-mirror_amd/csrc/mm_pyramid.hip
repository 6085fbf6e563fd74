// mm_pyramid.hip -- renders blended into backgrounds through a three-level Laplacian pyramid, as 8-bit frames, for gfx950: what the
// reference's tool/generate_market_test.py:326-369 does on the host, one image at a time, after every render (nine GaussianBlur calls that
// each draw their own sigma, four differences, a six-term blend, np.uint8(x * 255) behind a blocking .cpu()), one launch per batch of frames.
//
// A frame o is made of seven PLANES of three KINDS -- 0 the mask (channel 3 of render fg_index[o]), 1 a colour plane of background
// bg_index[o], 2 a colour plane of the render -- and every plane goes through the same CASCADE of MM_PYRAMID_LEVELS = 3 blurs, level l
// with the frame's own taps[kind][l - 1].  Each blur reflects at the image's own edge and rounds as written, and the blend reads every
// level, so every level is made in full.  Every step is fp32, rounded as written, sums taken in ascending tap index from 0, no contraction:
//   level 0   m0 = channel 3 of the render, obj0_c = channel c of the render, untouched.
//             bg0_c = channel c of the background behind the reflection pad (left, right, top, bottom) -- a virtual image (Hp,Wp) that is
//             index arithmetic only --, resized to (H,W) by the host's tap tables, x first, then y, NO blur before it:
//   hresize   g[y][x] = sum_t fl(wx[x][t] * v[y][C(sx[x] + t)])      C clamps to [0, Wp)
//   vresize   z[y][x] = sum_t fl(wy[y][t] * g[C(sy[y] + t)][x])      C clamps to [0, Hp)
//   level l   v_l = vblur(hblur(v_{l-1}, k), k), k = taps[kind][l - 1], r = (k - 1) / 2, both reflecting at the (H,W) image's own edge:
//   hblur     h[y][x] = sum_j fl(k[j] * v[y][R(x + j - r)])          R reflects at W
//   vblur     b[y][x] = sum_j fl(k[j] * h[R(y + j - r)][x])          R reflects at H
//   blend     t = fl(bg3 * fl(1 - m3));                     t = fl(t + fl(obj3 * m3))
//             t = fl(t + fl(fl(bg1 - bg2) * fl(1 - m2)));   t = fl(t + fl(fl(obj1 - obj2) * m2))
//             t = fl(t + fl(fl(bg0 - bg1) * fl(1 - m1)));   t = fl(t + fl(fl(obj0 - obj1) * m1))
//             then mm_export.hip's quantiser (mm_quant.h): the sums leave [0, 1]; it saturates and sends NaN to 0.
// A one-tap kernel {1.0} makes a level the identity and a resize row {i, 1, 1.0} makes the resize the identity, so there is one code path.
//
// One workgroup of 256 makes MM_PYRAMID_ROWS = 8 output rows [y0, y1) of one frame, plane after plane, in LDS.  Level 3 of a plane is
// needed on the band's rows, level l - 1 on the rows of level l widened by the radius r, clamped to [0, H): rows[l] below.  A row read through
// the reflect index always falls inside the clamped range (an index below 0 reflects to at most r - lo <= r, which is below hi + r; likewise
// at the other edge), so the band stages 8 + 6r rows of level 0 at most -- 8 + 18 at kernel 7 -- and neighbouring bands recompute the halo.
// Two row buffers A and T ping-pong: level l - 1 in A, its hblur in T, the vblur back into A (the rows of level l, from A's start) and, for the
// band's own rows, into the plane's KEEP slot.  The mask goes first and keeps m1..m3; then, per colour channel, the background (hresize from
// memory into T, vresize into A, which also keeps bg0) and the render cascades keep bg0..bg3 and obj1..obj3 (obj0 is read from memory again)
// and the blend reads the ten planes in the stated order.  Every pass has x along the lanes: a lane's column-wise taps step by whole rows,
// its neighbours read the neighbouring words, so no pass has a bank conflict.  The index maps, the resize rows and their sums, the render
// accessor and the band's bytes (their LDS layout and their way out) are mm_frame.h's, shared with mm_composite.hip; here are the level
// rows, the cascade, the keep slots and the blend.  Nothing intermediate goes to memory; no workspace, no atomics, no scratch; every
// output byte is written by one lane (bitwise reproducible).  Dynamic LDS only: 4 * (2 * cap + 10 * bw) + bytes, cap = the most rows any band stages (level 0's, or the resize's
// source rows) times W, bw = 8 * W, all rounded to 16 bytes.  MM_PYRAMID_MAX_KERNEL is 15: LDS does not force less -- kernel 15 at 128 x 128
// behind a pad of 16 takes 107 KiB, kernel 7 at 256 x 256 148 KiB -- and a call that needs more than 160 KiB is refused.
// The kernel has two instances: kernel size 7, the call site's, at compile time (its tap loops unroll), and the general one.
#include <hip/hip_runtime.h>

#include "mm_frame.h"

#define MM_PW MM_FRAME_ROW_WORDS
#define MM_PYR_KEEP 10                                        // m1 m2 m3 | bg0 bg1 bg2 bg3 | obj1 obj2 obj3

namespace mm {

struct PyrArgs {
    const float* fg; const float* bg; const int* par; void* out;
    int B, H, W, n_fg, n_bg, bgC, nhwc, k, pl, pr, pt, pb, nearest, as_float;
    int cap;                                                  // floats in each of the two row buffers
    int bw;                                                   // floats in a keep slot
    int nbands;
};

// where the tables lie in MMPyramidDesc.params (32-bit words)
struct PyrLayout { long long fg_index, bg_index, taps, bg_y, bg_x, words; };
__host__ __device__ inline PyrLayout pyramid_layout(int B, int H, int W, int k) {
    PyrLayout l;
    l.fg_index = 0; l.bg_index = B;
    l.taps = 2LL * B;
    l.bg_y = l.taps + 9LL * B * k; l.bg_x = l.bg_y + (long long)MM_PW * H;
    l.words = l.bg_x + (long long)MM_PW * W;
    return l;
}

// the rows [lo[l], hi[l]) of level l that the band [y0, y1) needs
struct PyrRows { int lo[MM_PYRAMID_LEVELS + 1], hi[MM_PYRAMID_LEVELS + 1]; };
__host__ __device__ inline PyrRows pyramid_rows(int y0, int y1, int r, int H) {
    PyrRows R;
    R.lo[MM_PYRAMID_LEVELS] = y0; R.hi[MM_PYRAMID_LEVELS] = y1;
#pragma unroll
    for (int l = MM_PYRAMID_LEVELS; l > 0; --l) {
        R.lo[l - 1] = R.lo[l] - r > 0 ? R.lo[l] - r : 0;
        R.hi[l - 1] = R.hi[l] + r < H ? R.hi[l] + r : H;
    }
    return R;
}

// level 0 of a plane lies in A on rows [R.lo[0], R.hi[0]); leaves levels 1..3 of the band's rows in keep[0], keep[bw], keep[2 bw].
// K: the kernel size at compile time (the tap loops unroll: the taps arrive in one scalar load and a lane's LDS reads are issued together,
// where the run-time loop waits for every tap's read in turn), or 0 for the size in a.k.  The order of the sums is the same.
template <int K>
__device__ inline void pyramid_cascade(const PyrArgs& a, const PyrRows& R, const float* taps, float* A, float* T, float* keep, int y0, int y1) {
    MM_FP_EXACT
    const int tid = threadIdx.x, W = a.W, H = a.H, k = K > 0 ? K : a.k, r = k >> 1;
#pragma unroll
    for (int l = 1; l <= MM_PYRAMID_LEVELS; ++l) {
        const float* tp = taps + (l - 1) * k;
        const int lo_in = R.lo[l - 1], n_in = R.hi[l - 1] - lo_in, lo = R.lo[l], n = R.hi[l] - lo;
        for (int i = tid; i < n_in * W; i += MM_FRAME_BLOCK) {  // horizontal blur of level l - 1
            const int row = i / W, x = i - row * W;
            const float* s = A + row * W;
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < k; ++j) acc = acc + tp[j] * s[reflecti(x + j - r, W)];
            T[i] = acc;
        }
        __syncthreads();
        for (int i = tid; i < n * W; i += MM_FRAME_BLOCK) {     // vertical blur: row y of level l reads rows R(y - r .. y + r) of level l - 1
            const int row = i / W, x = i - row * W, y = lo + row;
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < k; ++j) acc = acc + tp[j] * T[clampi(reflecti(y + j - r, H) - lo_in, 0, n_in - 1) * W + x];
            if (l < MM_PYRAMID_LEVELS) A[i] = acc;
            if (y >= y0 && y < y1) keep[(l - 1) * a.bw + (y - y0) * W + x] = acc;
        }
        __syncthreads();
    }
}

template <int K>
__global__ __launch_bounds__(MM_FRAME_BLOCK) void pyramid_blend_kernel(PyrArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = a.H, W = a.W, bw = a.bw;
    float* A = (float*)smem;
    float* T = A + a.cap;
    float* KM = T + a.cap;                                    // [3][bw] m1 m2 m3 of the band
    float* KB = KM + 3 * bw;                                  // [4][bw] bg0 .. bg3
    float* KO = KB + 4 * bw;                                  // [3][bw] obj1 .. obj3
    unsigned char* bytes = (unsigned char*)(KO + 3 * bw);

    const int tid = threadIdx.x;
    const int o = blockIdx.x / a.nbands, band = blockIdx.x - o * a.nbands;
    const int y0 = band * MM_PYRAMID_ROWS, y1 = min(y0 + MM_PYRAMID_ROWS, H);
    const int k = K > 0 ? K : a.k;
    const PyrLayout l = pyramid_layout(a.B, H, W, k);
    const long long fi = frame_index(a.par + l.fg_index, o, a.n_fg), bi = frame_index(a.par + l.bg_index, o, a.n_bg);
    const long long HW = (long long)H * W;
    const FrameFg fg_at = {a.fg + fi * 4 * HW, HW, W, a.nhwc};
    const float* taps = (const float*)(a.par + l.taps) + (long long)o * 9 * k;       // [kind][level][k]
    const PyrRows R = pyramid_rows(y0, y1, k >> 1, H);
    const int lo0 = R.lo[0], n0 = R.hi[0] - lo0;
    const int Hp = H + a.pt + a.pb, Wp = W + a.pl + a.pr, pl = a.pl;
    const int* ty = a.par + l.bg_y;
    const int* tx = a.par + l.bg_x;
    int c_lo, nsrc;
    frame_src_rows(ty, lo0, R.hi[0], 0, Hp, c_lo, nsrc);      // the rows of the virtual background that level 0's vertical resize reads
    if ((long long)(nsrc > n0 ? nsrc : n0) * W > a.cap) return;   // (uniform) a device table that is not the one the host sized the LDS from

    for (int i = tid; i < n0 * W; i += MM_FRAME_BLOCK) {        // the mask
        const int row = i / W, x = i - row * W;
        A[i] = fg_at(3, lo0 + row, x);
    }
    __syncthreads();
    pyramid_cascade<K>(a, R, taps, A, T, KM, y0, y1);

    unsigned char* g = (unsigned char*)a.out + ((long long)o * H + y0) * W * 3;     // the band's bytes (bytes mode)
    const int al = (int)((uintptr_t)g & 15);
    float* outf = (float*)a.out;
    for (int c = 0; c < 3; ++c) {
        const float* bgp = a.bg + (bi * a.bgC + c) * HW;
        for (int i = tid; i < nsrc * W; i += MM_FRAME_BLOCK) {  // background: horizontal resize of the padded rows, straight from memory
            const int row = i / W, x = i - row * W;
            const float* s = bgp + (long long)reflecti(c_lo + row - a.pt, H) * W;
            T[i] = frame_resize_sum(tx, x, 0, [=](int j) { return s[reflecti(clampi(j, 0, Wp - 1) - pl, W)]; });
        }
        __syncthreads();
        for (int i = tid; i < n0 * W; i += MM_FRAME_BLOCK) {    // vertical resize: level 0 of the background
            const int row = i / W, x = i - row * W, y = lo0 + row;
            const float acc = frame_resize_sum(ty, y, 0, [=](int j) { return T[clampi(clampi(j, 0, Hp - 1) - c_lo, 0, nsrc - 1) * W + x]; });
            A[i] = acc;
            if (y >= y0 && y < y1) KB[(y - y0) * W + x] = acc;
        }
        __syncthreads();
        pyramid_cascade<K>(a, R, taps + 3 * k, A, T, KB + bw, y0, y1);
        for (int i = tid; i < n0 * W; i += MM_FRAME_BLOCK) {    // the render's plane
            const int row = i / W, x = i - row * W;
            A[i] = fg_at(c, lo0 + row, x);
        }
        __syncthreads();
        pyramid_cascade<K>(a, R, taps + 6 * k, A, T, KO, y0, y1);
        for (int i = tid; i < (y1 - y0) * W; i += MM_FRAME_BLOCK) {
            MM_FP_EXACT
            const int yo = i / W, x = i - yo * W, y = y0 + yo;
            const float m1 = KM[i], m2 = KM[bw + i], m3 = KM[2 * bw + i];
            const float bg0 = KB[i], bg1 = KB[bw + i], bg2 = KB[2 * bw + i], bg3 = KB[3 * bw + i];
            const float obj0 = fg_at(c, y, x), obj1 = KO[i], obj2 = KO[bw + i], obj3 = KO[2 * bw + i];
            float t = bg3 * (1.0f - m3);
            t = t + obj3 * m3;
            t = t + (bg1 - bg2) * (1.0f - m2);
            t = t + (obj1 - obj2) * m2;
            t = t + (bg0 - bg1) * (1.0f - m1);
            t = t + (obj0 - obj1) * m1;
            frame_store_pixel(t, a.nearest, a.as_float, outf, o, c, y, x, H, W, bytes, al, i);
        }
        // (the next channel's first write to a keep slot lies behind a barrier that every lane reaches after this loop)
    }
    if (a.as_float) return;
    __syncthreads();                                          // the band's bytes are all in LDS
    frame_flush_bytes(g, bytes, al, (y1 - y0) * W * 3, tid);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// the bytes of LDS a call needs, from the host's copy of the tables: two row buffers for the tallest band (level 0's rows, or the rows
// its vertical resize reads), ten keep slots, the band's bytes at any 16-byte phase.  Fills the carving of `a`.
long long pyramid_lds_bytes(const MMPyramidDesc* d, PyrArgs* a) {
    const PyrLayout l = pyramid_layout(d->B, d->H, d->W, d->k);
    const int Hp = d->H + d->bg_pad[2] + d->bg_pad[3];
    long long rows = 0;
    for (int y0 = 0; y0 < d->H; y0 += MM_PYRAMID_ROWS) {
        const int y1 = y0 + MM_PYRAMID_ROWS < d->H ? y0 + MM_PYRAMID_ROWS : d->H;
        const PyrRows R = pyramid_rows(y0, y1, d->k >> 1, d->H);
        int c_lo, n;
        frame_src_rows(d->params_host + l.bg_y, R.lo[0], R.hi[0], 0, Hp, c_lo, n);
        const int n0 = R.hi[0] - R.lo[0];
        rows = n > rows ? n : rows;
        rows = n0 > rows ? n0 : rows;
    }
    const long long cap = (rows * d->W + 3) & ~3LL;
    const long long bw = ((long long)MM_PYRAMID_ROWS * d->W + 3) & ~3LL;
    if (a) { a->cap = cap < 0x7fffffff ? (int)cap : 0x7fffffff; a->bw = (int)bw; }
    return 4 * (2 * cap + MM_PYR_KEEP * bw) + frame_band_bytes_lds(MM_PYRAMID_ROWS, d->W);
}

int launch_pyramid(const MMPyramidDesc* d, hipStream_t s) {
    PyrArgs a = {};
    a.fg = d->renders; a.bg = d->backgrounds; a.par = d->params; a.out = d->out;
    a.B = d->B; a.H = d->H; a.W = d->W; a.n_fg = d->n_fg; a.n_bg = d->n_bg; a.bgC = d->bg_C; a.nhwc = d->fg_nhwc != 0; a.k = d->k;
    a.pl = d->bg_pad[0]; a.pr = d->bg_pad[1]; a.pt = d->bg_pad[2]; a.pb = d->bg_pad[3];
    a.nearest = d->rounding; a.as_float = d->as_float != 0;
    a.nbands = (d->H + MM_PYRAMID_ROWS - 1) / MM_PYRAMID_ROWS;
    const long long lds = pyramid_lds_bytes(d, &a);
    // kernel 7 is the call site's (tool/generate_market_test.py:330) and has its own instance; every other size runs the general one
    void (*const kernel)(PyrArgs) = d->k == 7 ? pyramid_blend_kernel<7> : pyramid_blend_kernel<0>;
    if (allow_large_lds((const void*)kernel, lds, MM_FRAME_LDS, "pyramid_lds") != MM_OK) return MM_ERR_LAUNCH;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(d->B * a.nbands)), dim3(MM_FRAME_BLOCK), (size_t)lds, s, a);
    return launch_ok("pyramid");
}

}  // namespace mm
