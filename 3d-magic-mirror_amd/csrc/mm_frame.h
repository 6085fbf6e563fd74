// mm_frame.h -- what the frame makers share (mm_composite.hip, mm_pyramid.hip): one workgroup of MM_FRAME_BLOCK makes MM_FRAME_ROWS output
// rows of one frame, plane after plane, in two LDS row buffers that the stages ping-pong between.  A background sits behind a reflection
// pad that is index arithmetic only (reflecti); a resize reads rows {start, n, w[MM_FRAME_MAX_TAPS]} of MM_FRAME_ROW_WORDS words that the
// host made (frame_src_rows, frame_resize_sum); a frame names its render and its background by index (frame_index, FrameFg); a band's bytes
// are one contiguous piece of the output, laid out in LDS at the output's own 16-byte phase (frame_store_pixel, frame_band_bytes_lds) and
// leaving as 16-byte stores (frame_flush_bytes).  Every sum is fp32, rounded as written, in ascending tap index from 0.
#pragma once
#include "mm_device.h"
#include "mm_quant.h"

#define MM_FRAME_BLOCK 256
#define MM_FRAME_LDS (160 * 1024)
#define MM_FRAME_ROWS MM_COMPOSITE_ROWS
#define MM_FRAME_MAX_TAPS MM_COMPOSITE_MAX_TAPS
#define MM_FRAME_ROW_WORDS MM_COMPOSITE_ROW_WORDS
static_assert(MM_PYRAMID_ROWS == MM_FRAME_ROWS && MM_PYRAMID_MAX_TAPS == MM_FRAME_MAX_TAPS && MM_PYRAMID_ROW_WORDS == MM_FRAME_ROW_WORDS, "one band, one resize row");

namespace mm {

__host__ __device__ inline int clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }
// a reflection pad or blur radius narrower than the dimension (the entry point holds them to that) reflects once
__host__ __device__ inline int reflecti(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return clampi(i, 0, n - 1);
}

// the source rows [c_lo, c_lo + n) of an axis of Hv that the vertical resize taps of output rows [y0, y1) read through a replicate pad of p
__host__ __device__ inline void frame_src_rows(const int* ty, int y0, int y1, int p, int Hv, int& c_lo, int& n) {
    int lo = 0x7fffffff, hi = -0x7fffffff;
    for (int y = y0; y < y1; ++y) {
        const int s = ty[y * MM_FRAME_ROW_WORDS], e = s + clampi(ty[y * MM_FRAME_ROW_WORDS + 1], 1, MM_FRAME_MAX_TAPS);
        lo = s < lo ? s : lo; hi = e > hi ? e : hi;
    }
    c_lo = clampi(lo - p, 0, Hv - 1);
    n = clampi(hi - 1 - p, 0, Hv - 1) - c_lo + 1;
}

// output index i of a resize through a replicate pad of p: sum_q fl(w[q] * at(start - p + q)) over row i of `table`; at(j) clamps j itself
template <class At>
__device__ inline float frame_resize_sum(const int* table, int i, int p, At at) {
    MM_FP_EXACT
    const int* t = table + i * MM_FRAME_ROW_WORDS;
    const int s0 = t[0] - p, n = clampi(t[1], 1, MM_FRAME_MAX_TAPS);
    float acc = 0.0f;
    for (int q = 0; q < n; ++q) acc = acc + __int_as_float(t[2 + q]) * at(s0 + q);
    return acc;
}

// entry o of an index table.  The entry point checked the host's copy; a device copy that differs reads another image, never a wild address
__device__ inline long long frame_index(const int* table, int o, int n) { return clampi(table[o], 0, n - 1); }

// channel c of a render (4,H,W) or (H,W,4) at pixel (y, x)
struct FrameFg {
    const float* p; long long HW; int W, nhwc;
    __device__ float operator()(int c, int y, int x) const {
        const long long i = (long long)y * W + x;
        return nhwc ? p[i * 4 + c] : p[c * HW + i];
    }
};

// pixel `pix` of the band, channel c, image row y: mm_export.hip's quantiser, then the float plane, or the byte in the band at phase al
__device__ inline void frame_store_pixel(float v, int nearest, int as_float, float* outf, int o, int c, int y, int x, int H, int W,
                                         unsigned char* bytes, int al, int pix) {
    const unsigned q = quant(v, nearest);
    if (as_float) outf[(((long long)o * 3 + c) * H + y) * W + x] = unquant(q);
    else bytes[al + pix * 3 + c] = (unsigned char)q;
}

// the band's n bytes, in LDS at bytes + al (al = g & 15), to g: the bytes before the first aligned chunk, 16-byte chunks, the bytes after
__device__ inline void frame_flush_bytes(unsigned char* g, const unsigned char* bytes, int al, int n, int tid) {
    int head = (16 - al) & 15;
    if (head > n) head = n;
    const int nch = (n - head) >> 4, done = head + nch * 16;
    const unsigned char* band = bytes + al;
    for (int j = tid; j < nch; j += MM_FRAME_BLOCK) *(uint4*)(g + head + 16 * j) = *(const uint4*)(band + head + 16 * j);
    if (tid < head) g[tid] = band[tid];
    if (tid >= 16 && tid - 16 < n - done) g[done + tid - 16] = *(band + done + tid - 16);
}

// LDS for the bytes of a band of `rows` rows at any 16-byte phase
__host__ __device__ inline long long frame_band_bytes_lds(int rows, int W) { return ((long long)rows * W * 3 + 16 + 15) & ~15LL; }

}  // namespace mm
