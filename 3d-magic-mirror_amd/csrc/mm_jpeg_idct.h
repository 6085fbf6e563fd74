// mm_jpeg_idct.h -- the back half of libjpeg's baseline decoder, stated once for the round trip (mm_jpeg.hip) and the file decoder
// (mm_jpeg_decode.hip): what an MCU is, where one image's sample planes lie, the zigzag order, a block to its row bytes (dequantise, jidctint's
// islow passes, the clamp), a pixel from the planes ("fancy" chroma upsampling, fixed-point YCbCr -> RGB), an output dword from its pixels.
// Their kernels keep what differs: how a lane finds its block, image and quantiser, and where the planes are.  Integer arithmetic only (>> is
// arithmetic); the order of every statement is pinned to Pillow to the byte by tests/test_gpu_jpeg_roundtrip.py, tests/test_gpu_jpeg_modes.py
// and tests/test_gpu_jpeg_decode.py -- see the round trip's header in mm_jpeg.hip for the formulas.
#pragma once
#include <hip/hip_runtime.h>

namespace mm {

enum { MM_JPG_420 = 0, MM_JPG_422 = 1, MM_JPG_444 = 2, MM_JPG_GREY = 3 };
template <int L>
struct JpegMcu {
    static_assert(L >= MM_JPG_420 && L <= MM_JPG_GREY, "a layout");
    static constexpr int LH_SHIFT = L <= MM_JPG_422 ? 1 : 0, LH = 1 << LH_SHIFT, LV = L == MM_JPG_420 ? 2 : 1;      // luma blocks across and down
    static constexpr int LUMA = LH * LV, BLOCKS = L == MM_JPG_GREY ? 1 : LUMA + 2;
    static constexpr int W = 8 * LH, H = 8 * LV;              // the MCU in pixels
    static constexpr int CHANNELS = L == MM_JPG_GREY ? 1 : 3; // bytes a pixel of the input
};
// the same at run time: blocks per MCU, luma blocks of them, the MCU in pixels
struct JpegMcuShape { int blocks, luma, w, h; };
template <int L>
__host__ __device__ constexpr JpegMcuShape jpeg_mcu_shape_of() { return {JpegMcu<L>::BLOCKS, JpegMcu<L>::LUMA, JpegMcu<L>::W, JpegMcu<L>::H}; }
__host__ __device__ inline JpegMcuShape jpeg_mcu_shape(int layout) {
    switch (layout) {
        case MM_JPG_420: return jpeg_mcu_shape_of<MM_JPG_420>();
        case MM_JPG_422: return jpeg_mcu_shape_of<MM_JPG_422>();
        case MM_JPG_444: return jpeg_mcu_shape_of<MM_JPG_444>();
        default: return jpeg_mcu_shape_of<MM_JPG_GREY>();
    }
}

// The padded sample planes of ONE image of mys x mxs MCUs: Y, 8 LV mys rows of 8 LH mxs bytes, at y; Cb then Cr, 8 mys rows of 8 mxs bytes each,
// at c (a greyscale image has none).  The IDCT kernels store through it, the pixel passes read through it.  An image has at most
// MM_JPEG_MAX_BLOCKS = 2^20 blocks (both callers' descriptors are refused beyond), so an offset inside its planes fits 32 bits.
struct JpegPlanes {
    unsigned char* y; unsigned char* c;
    int mxs, mys;
    __host__ __device__ static long long luma_bytes(const JpegMcuShape& m, long long mcus) { return mcus * m.w * m.h; }
    __host__ __device__ static long long chroma_bytes(const JpegMcuShape& m, long long mcus) { return m.blocks > m.luma ? mcus * 128 : 0; }
    // byte x of luma row `row`, in planes of MCUs mw pixels wide; of row `row` of chroma component comp (0: Cb, 1: Cr)
    __device__ unsigned char* luma(int mw, int row, int x) const { return y + ((unsigned)row * (unsigned)(mxs * mw) + x); }
    __device__ unsigned char* chroma(int comp, int row, int x) const { return c + ((unsigned)(comp * mys * 8 + row) * (unsigned)(mxs * 8) + x); }
};

// natural index -> position in zigzag order
__device__ const unsigned char jpeg_zigzag_pos[64] = {
    0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// one pass of jidctint over eight values, descaled by N bits
template <int N>
__device__ inline void jpeg_idct8(const int (&i)[8], int (&o)[8]) {
    constexpr int R = 1 << (N - 1);
    int z1 = (i[2] + i[6]) * 4433;
    const int t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
    const int t0 = (i[0] + i[4]) * (1 << 13), t1 = (i[0] - i[4]) * (1 << 13);
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
    z1 = a0 + a3;
    int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    o[0] = (t10 + a3 + R) >> N; o[7] = (t10 - a3 + R) >> N;
    o[1] = (t11 + a2 + R) >> N; o[6] = (t11 - a2 + R) >> N;
    o[2] = (t12 + a1 + R) >> N; o[5] = (t12 - a1 + R) >> N;
    o[3] = (t13 + a0 + R) >> N; o[4] = (t13 - a0 + R) >> N;
}

// a row after the row pass: + 128, clamped, as eight bytes in two words (byte c of the row at bits 8 * (c % 4) of word c / 4)
__device__ inline uint2 jpeg_row_bytes(const int (&o)[8]) {
    unsigned w[2] = {0u, 0u};
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c >> 2] |= (unsigned)min(max(o[c] + 128, 0), 255) << (8 * (c & 3));
    return make_uint2(w[0], w[1]);
}

// lane r (of the eight of block lb) holds column r after the column pass in o: the transpose, the row pass, row r as bytes.
// Every lane of the workgroup calls it; tile may still be read from before.
__device__ inline uint2 jpeg_idct_rows(int (*tile)[65], int lb, int r, int (&o)[8]) {
    int d[8];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[lb][k * 8 + r] = o[k];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 8; ++c) d[c] = tile[lb][r * 8 + c];
    jpeg_idct8<18>(d, o);
    return jpeg_row_bytes(o);
}

// A block to its row bytes: the eight lanes of block lb bring the 64 int16 zigzag coefficients at coef into zz, lane r dequantises column r
// by table()[nat] >> SHIFT (the table in natural order; the round trip's holds 8 q) and runs the column pass, then jpeg_idct_rows.  Every
// lane of the workgroup calls it; a lane that is not live reads nothing and transforms zeros.
template <int SHIFT, class T>
__device__ inline uint2 jpeg_block_rows(int (*tile)[65], short (*zz)[64], int lb, int r, bool live, const short* coef, T table) {
    if (live) *(uint4*)&zz[lb][r * 8] = *(const uint4*)(coef + r * 8);
    __syncthreads();
    const int* q = table();
    int d[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int nat = k * 8 + r;
        d[k] = live ? (int)zz[lb][jpeg_zigzag_pos[nat]] * (q[nat] >> SHIFT) : 0;
    }
    jpeg_idct8<11>(d, o);
    return jpeg_idct_rows(tile, lb, r, o);
}

// the upsampled chroma sample at (y, x) of one component's plane c (cw bytes a row), real on hd rows by wd columns
template <int L>
__device__ inline int jpeg_chroma_up_at(const unsigned char* c, size_t cw, int y, int x, int hd, int wd) {
    if constexpr (L == MM_JPG_444) return c[y * cw + x];      // no upsampling
    if constexpr (L == MM_JPG_422) {                          // h2v1: no vertical neighbour
        const int cx = x >> 1;
        const unsigned char* p = c + y * cw;
        if (wd <= 2) return p[cx];
        const int ox = (x & 1) ? min(cx + 1, wd - 1) : max(cx - 1, 0);
        return (3 * p[cx] + p[ox] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int r = y >> 1, cx = x >> 1;
    const unsigned char* p = c + r * cw;
    if (wd <= 2) return p[cx];
    const unsigned char* q = c + ((y & 1) ? min(r + 1, hd - 1) : max(r - 1, 0)) * cw;
    const int ox = (x & 1) ? min(cx + 1, wd - 1) : max(cx - 1, 0);
    const int s = 3 * p[cx] + q[cx], so = 3 * p[ox] + q[ox];
    return (3 * s + so + ((x & 1) ? 7 : 8)) >> 4;
}

// Y and the chroma samples minus 128 as one pixel: R | G << 8 | B << 16
__device__ inline unsigned jpeg_ycc_rgb(int Y, int cb, int cr) {
    const int R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
    const int G = min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
    const int B = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
    return (unsigned)R | (unsigned)G << 8 | (unsigned)B << 16;
}

// the pixel at (y, x) of the image whose planes are pl, its chroma real on hd rows by wd columns: R | G << 8 | B << 16
template <int L>
__device__ inline unsigned jpeg_pixel_at(const JpegPlanes& pl, int hd, int wd, int y, int x) {
    const size_t cw = (size_t)pl.mxs * 8;
    const int Y = *pl.luma(JpegMcu<L>::W, y, x);
    const int cb = jpeg_chroma_up_at<L>(pl.chroma(0, 0, 0), cw, y, x, hd, wd) - 128, cr = jpeg_chroma_up_at<L>(pl.chroma(1, 0, 0), cw, y, x, hd, wd) - 128;
    return jpeg_ycc_rgb(Y, cb, cr);
}

// bytes [first, last) of a dense output, at most the four of one aligned dword, out of w (byte `first` at bits 0..7): one 4-byte store, or
// the byte tail at the output's two ends
__device__ inline void jpeg_store_bytes(unsigned char* out, long long first, long long last, unsigned w) {
    out += first;
    if (last - first == 4) *(unsigned*)out = w;
    else for (int k = 0; k < (int)(last - first); ++k) out[k] = (unsigned char)(w >> (8 * k));
}
// that w for bytes [first, last) of an RGB output, pixel(p) giving its pixel p as R | G << 8 | B << 16: the six bytes of pixels p and p + 1, shifted to `first`
template <class P>
__device__ inline unsigned jpeg_rgb_bytes(long long first, long long last, P pixel) {
    const long long p = first / 3;
    unsigned long long seq = pixel(p);
    if (3 * (p + 1) < last) seq |= (unsigned long long)pixel(p + 1) << 24;
    return (unsigned)(seq >> (8 * (int)(first - 3 * p)));
}

}  // namespace mm
