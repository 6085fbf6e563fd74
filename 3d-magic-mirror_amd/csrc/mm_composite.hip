// mm_composite.hip -- renders composed over blurred backgrounds as 8-bit frames, for gfx950: what the reference's dataset-generation scripts do
// on the host, one image at a time, after every render (generate_market++.py:308-349, generate_market_new_class9.py:323-347,
// tool/generate_market.py:293-313: makeup_hole, GaussianBlur of the mask, ReplicationPad2d + Resize, ReflectionPad2d + GaussianBlur + Resize of a
// random background, blend, np.uint8(x * 255)), one launch per batch of frames.
//
// A frame o is made of four PLANES that go through one pipeline (run_plane): the mask (channel 3 of render fg_index[o]) and the three colour
// planes of background bg_index[o].  A plane is a VIRTUAL source (Hv,Wv) -- the image behind a reflection pad, which is index arithmetic and
// is never materialised; the mask has no such pad, and its source value may be the hole-filled one --, a blur with the frame's own taps that
// reflects at the virtual source's edge, a replicate pad p of the blurred plane (the mask's; 0 for a background), and a resize of
// (Hv + 2p, Wv + 2p) to (H,W) by the host's tap tables.  Every step is fp32, rounded as written, sums taken in ascending tap index from 0:
//   fill      s = (((0 + m[y-1][x-1]) + m[y-1][x]) + ... + m[y+1][x+1]) over the pixels inside the image, s = fl(s / 9); 1 if s > 0.7, 0 if s <= 0.7, else s (NaN)
//   hblur     h[y][x] = sum_j fl(k[j] * v[y][R(x + j - r)])          R reflects at Wv
//   vblur     b[y][x] = sum_j fl(k[j] * h[R(y + j - r)][x])          R reflects at Hv
//   hresize   g[y][x] = sum_t fl(wx[x][t] * b[y][C(sx[x] + t - p)])  C clamps to [0, Wv)
//   vresize   z[y][x] = sum_t fl(wy[y][t] * g[C(sy[y] + t - p)][x])  C clamps to [0, Hv)
//   blend     out_c = fl(fl(fg_c * m') + fl(bg'_c * fl(1 - m'))), then mm_export.hip's quantiser (mm_quant.h)
// A stage that a call does not use is the identity in this form (one tap of 1.0), so there is one code path.
//
// One workgroup of 256 makes MM_COMPOSITE_ROWS output rows of one frame, plane after plane, in two LDS row buffers that the stages
// ping-pong between: the source rows the band needs (the rows its vertical resize taps read, widened by the blur radius, reflected on the
// fly), hblur, vblur, hresize, then the vertical resize, whose result goes to an LDS plane (the mask) or straight into the blend (a
// background plane, quantised to a byte in LDS).  Every pass has x along the lanes: a lane's column-wise taps step by whole rows, its
// neighbours read the neighbouring words, so no pass has a bank conflict beyond the two-way one of a resize's stride.  Neighbouring bands
// recompute the halo rows.  Nothing intermediate goes to memory; no atomics, no workspace, no scratch; every output byte is written by one
// lane (bitwise reproducible).  The index maps, the resize rows and their sums, the render accessor and the band's bytes (their LDS layout
// and their way out) are mm_frame.h's, shared with mm_pyramid.hip; here are the hole fill, run_plane's order of stages and the blend.
#include <hip/hip_runtime.h>

#include "mm_frame.h"

#define MM_CW MM_FRAME_ROW_WORDS

namespace mm {

struct CompArgs {
    const float* fg; const float* bg; const int* par; void* out;
    int B, H, W, n_fg, n_bg, bgC, nhwc, fill, mk, bk, mpad, pl, pr, pt, pb, nearest, as_float;
    int cap;                                                  // floats in each of the two row buffers
    int nbands;
};

// where the tables lie in MMCompositeDesc.params (32-bit words)
struct CompLayout { long long fg_index, bg_index, mask_taps, bg_taps, mask_y, mask_x, bg_y, bg_x, words; };
__host__ __device__ inline CompLayout composite_layout(int B, int H, int W, int mk, int bk) {
    CompLayout l;
    l.fg_index = 0; l.bg_index = B;
    l.mask_taps = 2LL * B; l.bg_taps = l.mask_taps + (long long)B * mk;
    l.mask_y = l.bg_taps + (long long)B * bk; l.mask_x = l.mask_y + (long long)MM_CW * H;
    l.bg_y = l.mask_x + (long long)MM_CW * W; l.bg_x = l.bg_y + (long long)MM_CW * H;
    l.words = l.bg_x + (long long)MM_CW * W;
    return l;
}

struct Plane {
    int Hv, Wv;                                               // the virtual source: the image behind its reflection pad
    int pl, pt;                                               // the image's origin in it
    int k; const float* taps;                                 // this frame's blur taps
    int p;                                                    // replicate pad of the blurred plane
    const int* ty; const int* tx;                             // resize rows of the H output rows / W output columns
};

// src(y, x): the plane's value at image pixel (y, x); sink(yo, x, v): row yo of the band, column x
template <class Src, class Sink>
__device__ inline void run_plane(const CompArgs& a, const Plane& P, float* b0, float* b1, int y0, int y1, Src src, Sink sink) {
    MM_FP_EXACT
    const int tid = threadIdx.x, r = P.k >> 1, Hv = P.Hv, Wv = P.Wv, W = a.W;
    int c_lo, nvb;
    frame_src_rows(P.ty, y0, y1, P.p, Hv, c_lo, nvb);        // the blurred rows the band's vertical resize reads
    const int ns = nvb + 2 * r;
    if ((long long)ns * Wv > a.cap) return;                   // (uniform) a device table that is not the one the host sized the LDS from
    for (int i = tid; i < ns * Wv; i += MM_FRAME_BLOCK) { // source rows, reflected twice: at the virtual source's edge, then at the image's
        const int row = i / Wv, x = i - row * Wv;
        const int vy = reflecti(c_lo - r + row, Hv);
        b0[i] = src(reflecti(vy - P.pt, a.H), reflecti(x - P.pl, W));
    }
    __syncthreads();
    for (int i = tid; i < ns * Wv; i += MM_FRAME_BLOCK) { // horizontal blur
        const int row = i / Wv, x = i - row * Wv;
        const float* s = b0 + row * Wv;
        float acc = 0.0f;
        for (int j = 0; j < P.k; ++j) acc = acc + P.taps[j] * s[reflecti(x + j - r, Wv)];
        b1[i] = acc;
    }
    __syncthreads();
    for (int i = tid; i < nvb * Wv; i += MM_FRAME_BLOCK) {   // vertical blur: blurred row c_lo + row reads staged rows row .. row + 2r
        const float* s = b1 + i;
        float acc = 0.0f;
        for (int j = 0; j < P.k; ++j) acc = acc + P.taps[j] * s[j * Wv];
        b0[i] = acc;
    }
    __syncthreads();
    for (int i = tid; i < nvb * W; i += MM_FRAME_BLOCK) { // horizontal resize through the replicate pad
        const int row = i / W, x = i - row * W;
        const float* s = b0 + row * Wv;
        b1[i] = frame_resize_sum(P.tx, x, P.p, [=](int j) { return s[clampi(j, 0, Wv - 1)]; });
    }
    __syncthreads();
    for (int i = tid; i < (y1 - y0) * W; i += MM_FRAME_BLOCK) {   // vertical resize
        const int yo = i / W, x = i - yo * W;
        sink(yo, x, frame_resize_sum(P.ty, y0 + yo, P.p, [=](int j) { return b1[(clampi(j, 0, Hv - 1) - c_lo) * W + x]; }));
    }
    __syncthreads();
}

__global__ __launch_bounds__(MM_FRAME_BLOCK) void composite_kernel(CompArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = a.H, W = a.W;
    float* b0 = (float*)smem;
    float* b1 = b0 + a.cap;
    float* M = b1 + a.cap;                                    // [MM_COMPOSITE_ROWS][W] the band's finished mask
    unsigned char* bytes = (unsigned char*)(M + ((MM_COMPOSITE_ROWS * W + 3) & ~3));

    const int o = blockIdx.x / a.nbands, band = blockIdx.x - o * a.nbands;
    const int y0 = band * MM_COMPOSITE_ROWS, y1 = min(y0 + MM_COMPOSITE_ROWS, H);
    const CompLayout l = composite_layout(a.B, H, W, a.mk, a.bk);
    const long long fi = frame_index(a.par + l.fg_index, o, a.n_fg), bi = frame_index(a.par + l.bg_index, o, a.n_bg);
    const long long HW = (long long)H * W;
    const FrameFg fg_at = {a.fg + fi * 4 * HW, HW, W, a.nhwc};

    Plane P;
    P.Hv = H; P.Wv = W; P.pl = 0; P.pt = 0; P.k = a.mk; P.taps = (const float*)(a.par + l.mask_taps) + (long long)o * a.mk;
    P.p = a.mpad; P.ty = a.par + l.mask_y; P.tx = a.par + l.mask_x;
    const int fill = a.fill;
    run_plane(a, P, b0, b1, y0, y1,
              [=](int y, int x) -> float {
                  MM_FP_EXACT
                  if (!fill) return fg_at(3, y, x);
                  float s = 0.0f;
                  for (int dy = -1; dy <= 1; ++dy)
                      for (int dx = -1; dx <= 1; ++dx) {
                          const int yy = y + dy, xx = x + dx;
                          if (yy >= 0 && yy < H && xx >= 0 && xx < W) s = s + fg_at(3, yy, xx);
                      }
                  s = s / 9.0f;
                  return s > 0.7f ? 1.0f : (s <= 0.7f ? 0.0f : s);
              },
              [=](int yo, int x, float v) { M[yo * W + x] = v; });

    unsigned char* g = (unsigned char*)a.out + ((long long)o * H + y0) * W * 3;     // the band's bytes (bytes mode)
    const int al = (int)((uintptr_t)g & 15);
    P.Hv = H + a.pt + a.pb; P.Wv = W + a.pl + a.pr; P.pl = a.pl; P.pt = a.pt; P.k = a.bk;
    P.taps = (const float*)(a.par + l.bg_taps) + (long long)o * a.bk;
    P.p = 0; P.ty = a.par + l.bg_y; P.tx = a.par + l.bg_x;
    const int nearest = a.nearest, as_float = a.as_float;
    float* outf = (float*)a.out;
    for (int c = 0; c < 3; ++c) {
        const float* bgp = a.bg + (bi * a.bgC + c) * HW;
        run_plane(a, P, b0, b1, y0, y1,
                  [=](int y, int x) -> float { return bgp[(long long)y * W + x]; },
                  [=](int yo, int x, float v) {
                      MM_FP_EXACT
                      const int y = y0 + yo;
                      const float m = M[yo * W + x];
                      const float f = fg_at(c, y, x);
                      frame_store_pixel(f * m + v * (1.0f - m), nearest, as_float, outf, o, c, y, x, H, W, bytes, al, yo * W + x);
                  });
    }
    if (as_float) return;
    // (run_plane ended on a barrier: the band's bytes are all in LDS)
    frame_flush_bytes(g, bytes, al, (y1 - y0) * W * 3, threadIdx.x);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// the bytes of LDS a call needs, from the host's copy of the tables: two row buffers for the tallest, widest plane of any band, the
// band's mask, the band's bytes at any 16-byte phase.  Fills the carving of `a`.
long long composite_lds_bytes(const MMCompositeDesc* d, CompArgs* a) {
    const CompLayout l = composite_layout(d->B, d->H, d->W, d->mask_k, d->bg_k);
    const int Hp = d->H + d->bg_pad[2] + d->bg_pad[3], Wp = d->W + d->bg_pad[0] + d->bg_pad[1];
    long long cap = 0;
    for (int y0 = 0; y0 < d->H; y0 += MM_COMPOSITE_ROWS) {
        const int y1 = y0 + MM_COMPOSITE_ROWS < d->H ? y0 + MM_COMPOSITE_ROWS : d->H;
        int c_lo, n;
        frame_src_rows(d->params_host + l.mask_y, y0, y1, d->mask_pad, d->H, c_lo, n);
        const long long m = (long long)(n + d->mask_k - 1) * d->W;
        frame_src_rows(d->params_host + l.bg_y, y0, y1, 0, Hp, c_lo, n);
        const long long b = (long long)(n + d->bg_k - 1) * Wp;
        cap = m > cap ? m : cap;
        cap = b > cap ? b : cap;
    }
    cap = (cap + 3) & ~3LL;
    if (a) a->cap = cap < 0x7fffffff ? (int)cap : 0x7fffffff;
    const long long mw = ((long long)MM_COMPOSITE_ROWS * d->W + 3) & ~3LL;
    return 4 * (2 * cap + mw) + frame_band_bytes_lds(MM_COMPOSITE_ROWS, d->W);
}

int launch_composite(const MMCompositeDesc* d, hipStream_t s) {
    CompArgs a = {};
    a.fg = d->renders; a.bg = d->backgrounds; a.par = d->params; a.out = d->out;
    a.B = d->B; a.H = d->H; a.W = d->W; a.n_fg = d->n_fg; a.n_bg = d->n_bg; a.bgC = d->bg_C; a.nhwc = d->fg_nhwc != 0; a.fill = d->fill_holes != 0;
    a.mk = d->mask_k; a.bk = d->bg_k; a.mpad = d->mask_pad;
    a.pl = d->bg_pad[0]; a.pr = d->bg_pad[1]; a.pt = d->bg_pad[2]; a.pb = d->bg_pad[3];
    a.nearest = d->rounding; a.as_float = d->as_float != 0;
    a.nbands = (d->H + MM_COMPOSITE_ROWS - 1) / MM_COMPOSITE_ROWS;
    const long long lds = composite_lds_bytes(d, &a);
    if (allow_large_lds((const void*)composite_kernel, lds, MM_FRAME_LDS, "composite_lds") != MM_OK) return MM_ERR_LAUNCH;
    hipLaunchKernelGGL(composite_kernel, dim3((unsigned)(d->B * a.nbands)), dim3(MM_FRAME_BLOCK), (size_t)lds, s, a);
    return launch_ok("composite");
}

}  // namespace mm
