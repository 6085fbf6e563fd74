// mm_jpeg_decode.hip -- baseline JPEG FILES to 8-bit device frames, for gfx950: what the reference's datasets and evaluation do on the host
// per file with Image.open(f).convert('RGB') (datasets/market.py, atr.py, bird.py; test.py:430-463, trainer.py:771-836, fid_score.py:71-76).
// The front half of a decoder; the back half (block -> row bytes, planes -> pixel, pixels -> output dword) is mm_jpeg_idct.h, shared with the
// round trip and pinned to Pillow to the byte.  The caller parses the markers (jpeg_decode.py); the tables it hands over are described at
// MMJpegDecodeDesc in include/mm_render.h, and every record is re-checked here, on the host, before anything is launched (check_jpeg_decode).
//
// One memset (coefficients and status, adjacent in the workspace) and three launches, whatever the number of files:
//   entropy   one lane per SEGMENT -- a file, or one restart interval of it.  A workgroup is one wave; MM_JPEG_DEC_GROUP of its lanes take a
//             segment each, all of one table set; it stages the set's four Huffman tables (4 x 1424 bytes) into LDS, then every lane runs jpeg_decode_segment of
//             mm_jpeg_entropy.h: FF 00 unstuffing, DC prediction from 0, EOB / ZRL / EXTEND, one 2-byte store per non-zero coefficient
//             into the zeroed (blocks, 64) int16 zigzag buffer -- the layout the IDCT reads.  Latency-bound and divergent by nature; the
//             parallelism is the number of segments in flight.  A lane's status bits are ORed into its file's status word.
//   idct      eight lanes per block, over all files' blocks: the block's file by bisection of the records' first blocks, dequantise with
//             the file's own table of the block's component, column pass, transpose through LDS, row pass, row r as 8 bytes into the
//             file's padded sample planes.
//   pixels    one lane per aligned dword of the output, whatever byte `out` starts at: the two (RGB) or four (L) pixels it touches, each
//             with its file by bisection of the pixel offsets; upsample, convert, one 4-byte store -- byte stores at the output's two ends.
//             Files are packed without padding, so a dword may hold the end of one file and the start of the next.
// No floating point, no scratch; every output byte is a pure function of the files.
#include <hip/hip_runtime.h>

#include <cstring>

#include "mm_device.h"
#include "mm_jpeg_entropy.h"
#include "mm_jpeg_idct.h"
#include "mm_stream.h"                                        // Carve

#define MM_JPGD_BLOCK 256
#define MM_JPGD_WAVE 64

namespace mm {

// the words of a file record
enum { JD_H = 0, JD_W = 1, JD_LAYOUT = 2, JD_MX = 3, JD_MY = 4, JD_BLOCK0 = 5, JD_YOFF = 6, JD_COFF = 7, JD_Q0 = 8 };
enum { JS_FILE = 0, JS_FIRST = 1, JS_COUNT = 2, JS_BEGIN = 3, JS_END = 4, JS_SET = 5 };

struct JpegDecodeTables {                                     // where the tables lie in MMJpegDecodeDesc.tables (32-bit words)
    size_t files, offsets, segments, qtables, htables, sets, words;
};
__host__ JpegDecodeTables jpeg_decode_tables(const MMJpegDecodeDesc* d) {
    JpegDecodeTables t;
    t.files = 0;
    t.offsets = t.files + (size_t)d->n * MM_JPEG_DEC_FILE_INTS;
    t.segments = t.offsets + 2 * ((size_t)d->n + 1);
    t.qtables = t.segments + (size_t)d->n_segments * MM_JPEG_DEC_SEGMENT_INTS;
    t.htables = t.qtables + (size_t)d->n_qtables * 64;
    t.sets = t.htables + (size_t)d->n_htables * MM_JPEG_TABLE_WORDS;
    t.words = t.sets + (size_t)d->n_sets * MM_JPEG_DEC_SET_INTS;
    return t;
}

// totals of a call whose records passed check_jpeg_decode
struct JpegDecodeTotals { long long blocks, plane_bytes, pixels; };
__host__ JpegDecodeTotals jpeg_decode_totals(const MMJpegDecodeDesc* d) {
    const JpegDecodeTables t = jpeg_decode_tables(d);
    const int32_t* f = d->tables_host + t.files + (size_t)(d->n - 1) * MM_JPEG_DEC_FILE_INTS;
    const JpegMcuShape s = jpeg_mcu_shape(f[JD_LAYOUT]);
    const long long mcus = (long long)f[JD_MX] * f[JD_MY];
    JpegDecodeTotals r;
    r.blocks = f[JD_BLOCK0] + mcus * s.blocks;
    r.plane_bytes = f[JD_YOFF] + JpegPlanes::luma_bytes(s, mcus) + JpegPlanes::chroma_bytes(s, mcus);
    long long last;
    std::memcpy(&last, d->tables_host + t.offsets + 2 * (size_t)d->n, 8);
    r.pixels = last;
    return r;
}

struct JpegDecodeLayout { size_t coef, status, planes, bytes; };
__host__ JpegDecodeLayout jpeg_decode_layout(const MMJpegDecodeDesc* d) {
    const JpegDecodeTotals r = jpeg_decode_totals(d);
    JpegDecodeLayout l;
    Carve c;
    l.coef = c.take((size_t)r.blocks * 128);
    l.status = c.take((size_t)d->n * 4);
    l.planes = c.take((size_t)r.plane_bytes);
    l.bytes = c.at;
    return l;
}
size_t jpeg_decode_workspace_bytes(const MMJpegDecodeDesc* d) { return jpeg_decode_layout(d).bytes; }

// Every record of tables_host, before anything is launched: the kernels index with what these records say and with nothing else.
int check_jpeg_decode(const MMJpegDecodeDesc* d) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->n < 1 || d->n_segments < MM_JPEG_DEC_GROUP || d->n_segments % MM_JPEG_DEC_GROUP || d->n_qtables < 1 || d->n_htables < 1 || d->n_sets < 1 || d->n_bytes < 1)
        return MM_ERR_BAD_SHAPE;
    if (d->mode != MM_JPEG_MODE_RGB && d->mode != MM_JPEG_MODE_L) return MM_ERR_BAD_SHAPE;
    if (d->n > MM_JPEG_DEC_MAX_FILES || d->n_bytes > 0x7fffffffLL) return MM_ERR_UNSUPPORTED;
    if (!d->tables_host) return MM_ERR_NULL_POINTER;
    const JpegDecodeTables t = jpeg_decode_tables(d);
    const int32_t* tab = d->tables_host;
    long long block0 = 0, plane = 0, pixel = 0;
    for (int i = 0; i < d->n; ++i) {
        const int32_t* f = tab + t.files + (size_t)i * MM_JPEG_DEC_FILE_INTS;
        const int H = f[JD_H], W = f[JD_W], layout = f[JD_LAYOUT];
        if (H < 1 || W < 1 || H > 65535 || W > 65535 || layout < MM_JPG_420 || layout > MM_JPG_GREY) return MM_ERR_BAD_SHAPE;
        if (d->mode == MM_JPEG_MODE_L && layout != MM_JPG_GREY) return MM_ERR_BAD_SHAPE;
        const JpegMcuShape s = jpeg_mcu_shape(layout);
        if (f[JD_MX] != (W + s.w - 1) / s.w || f[JD_MY] != (H + s.h - 1) / s.h) return MM_ERR_BAD_SHAPE;
        const long long mcus = (long long)f[JD_MX] * f[JD_MY];
        if (mcus * s.blocks > MM_JPEG_MAX_BLOCKS) return MM_ERR_UNSUPPORTED;
        if (f[JD_BLOCK0] != block0 || f[JD_YOFF] != plane) return MM_ERR_BAD_SHAPE;
        block0 += mcus * s.blocks;
        plane += JpegPlanes::luma_bytes(s, mcus);
        if (f[JD_COFF] != (layout != MM_JPG_GREY ? plane : 0)) return MM_ERR_BAD_SHAPE;
        plane += JpegPlanes::chroma_bytes(s, mcus);
        if (block0 > MM_JPEG_DEC_MAX_BLOCKS) return MM_ERR_UNSUPPORTED;     // (so the planes, 64 bytes a block, stay below 2^31 too)
        for (int c = 0; c < 3; ++c) if (f[JD_Q0 + c] < 0 || f[JD_Q0 + c] >= d->n_qtables) return MM_ERR_BAD_SHAPE;
        long long at, next;
        std::memcpy(&at, tab + t.offsets + 2 * (size_t)i, 8);
        std::memcpy(&next, tab + t.offsets + 2 * (size_t)i + 2, 8);
        if (at != pixel || next != pixel + (long long)H * W) return MM_ERR_BAD_SHAPE;
        pixel = next;
    }
    for (int i = 0; i < d->n_segments; ++i) {
        const int32_t* s = tab + t.segments + (size_t)i * MM_JPEG_DEC_SEGMENT_INTS;
        if (s[JS_FILE] < 0 || s[JS_FILE] >= d->n || s[JS_SET] < 0 || s[JS_SET] >= d->n_sets) return MM_ERR_BAD_SHAPE;
        if (s[JS_SET] != tab[t.segments + (size_t)(i - i % MM_JPEG_DEC_GROUP) * MM_JPEG_DEC_SEGMENT_INTS + JS_SET]) return MM_ERR_BAD_SHAPE;
        const int32_t* f = tab + t.files + (size_t)s[JS_FILE] * MM_JPEG_DEC_FILE_INTS;
        const long long mcus = (long long)f[JD_MX] * f[JD_MY];
        if (s[JS_FIRST] < 0 || s[JS_COUNT] < 0 || (long long)s[JS_FIRST] + s[JS_COUNT] > mcus) return MM_ERR_BAD_SHAPE;
        if (s[JS_BEGIN] < 0 || s[JS_END] < s[JS_BEGIN] || s[JS_END] > d->n_bytes) return MM_ERR_BAD_SHAPE;
    }
    for (size_t i = 0; i < (size_t)d->n_qtables * 64; ++i) if (tab[t.qtables + i] < 1 || tab[t.qtables + i] > 255) return MM_ERR_BAD_SHAPE;
    for (int i = 0; i < d->n_sets; ++i) {
        const int32_t* s = tab + t.sets + (size_t)i * MM_JPEG_DEC_SET_INTS;
        for (int k = 0; k < 4; ++k) if (s[k] < 0 || s[k] >= d->n_htables) return MM_ERR_BAD_SHAPE;
    }
    return MM_OK;
}

struct JpegDecodeArgs {
    const unsigned char* bytes;
    const int* files; const long long* offsets; const int* segments; const int* qtables; const unsigned* htables; const int* sets;
    short* coef; int* status; unsigned char* planes; unsigned char* out;
    int n, channels;
    long long total_blocks, total_bytes;
};
__device__ inline JpegPlanes jpeg_decode_planes(const JpegDecodeArgs& a, const int* f) {      // the sample planes of the file whose record is f
    return {a.planes + (size_t)f[JD_YOFF], a.planes + (size_t)f[JD_COFF], f[JD_MX], f[JD_MY]};
}

// ---- entropy: segments -> coefficients ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_JPGD_WAVE) void jpeg_decode_entropy_kernel(JpegDecodeArgs a) {
    __shared__ unsigned tables[4 * MM_JPEG_TABLE_WORDS];
    const int tid = threadIdx.x;
    const int* seg0 = a.segments + (size_t)blockIdx.x * MM_JPEG_DEC_GROUP * MM_JPEG_DEC_SEGMENT_INTS;
    const int* set = a.sets + (size_t)seg0[JS_SET] * MM_JPEG_DEC_SET_INTS;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned* src = a.htables + (size_t)set[k] * MM_JPEG_TABLE_WORDS;
        for (int i = tid; i < MM_JPEG_TABLE_WORDS; i += MM_JPGD_WAVE) tables[k * MM_JPEG_TABLE_WORDS + i] = src[i];
    }
    __syncthreads();
    if (tid >= MM_JPEG_DEC_GROUP) return;                     // (the other lanes were there for the staging)
    const int* s = seg0 + tid * MM_JPEG_DEC_SEGMENT_INTS;
    const int count = s[JS_COUNT];
    if (count == 0) return;                                   // a filler
    const int* f = a.files + (size_t)s[JS_FILE] * MM_JPEG_DEC_FILE_INTS;
    const JpegMcuShape m = jpeg_mcu_shape(f[JD_LAYOUT]);
    short* coef = a.coef + ((size_t)f[JD_BLOCK0] + (size_t)s[JS_FIRST] * m.blocks) * 64;
    const int st = jpeg_decode_segment(a.bytes, s[JS_BEGIN], s[JS_END], tables, (unsigned)set[4], m.blocks, m.luma, count, coef);
    if (st) atomicOr(a.status + s[JS_FILE], st);
}

// ---- idct: coefficients -> the files' sample planes ----------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_JPGD_BLOCK) void jpeg_decode_idct_kernel(JpegDecodeArgs a) {
    __shared__ int tile[MM_JPGD_BLOCK / 8][65];
    __shared__ __attribute__((aligned(16))) short zz[MM_JPGD_BLOCK / 8][64];
    const int tid = threadIdx.x, lb = tid >> 3, r = tid & 7;
    const long long g = (long long)blockIdx.x * (MM_JPGD_BLOCK / 8) + lb;
    const bool live = g < a.total_blocks;
    const int gc = (int)(live ? g : 0);
    int lo = 0, hi = a.n - 1;                                 // the last file whose first block is <= gc
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.files[(size_t)mid * MM_JPEG_DEC_FILE_INTS + JD_BLOCK0] <= gc) lo = mid; else hi = mid - 1;
    }
    const int* f = a.files + (size_t)lo * MM_JPEG_DEC_FILE_INTS;
    const JpegPlanes pl = jpeg_decode_planes(a, f);
    const JpegMcuShape m = jpeg_mcu_shape(f[JD_LAYOUT]);
    const int rem = gc - f[JD_BLOCK0], mcu = rem / m.blocks, j = rem % m.blocks, my = mcu / pl.mxs, mx = mcu % pl.mxs;
    const uint2 row = jpeg_block_rows<0>(tile, zz, lb, r, live, a.coef + (size_t)g * 64,       // the file's own table of the block's component
                                         [&] { return a.qtables + (size_t)f[JD_Q0 + (j < m.luma ? 0 : j - m.luma + 1)] * 64; });
    if (!live) return;
    const int lh = m.w >> 3;                                  // luma blocks across an MCU
    if (j < m.luma) *(uint2*)pl.luma(m.w, ((m.h >> 3) * my + j / lh) * 8 + r, (lh * mx + j % lh) * 8) = row;
    else *(uint2*)pl.chroma(j - m.luma, my * 8 + r, mx * 8) = row;
}

// ---- pixels: upsample, convert, store -----------------------------------------------------------------------------------------------
// pixel p of the output (its file is `file` or a later one; `file` is moved on to it): R | G << 8 | B << 16, or the sample for one channel
__device__ inline unsigned jpeg_decode_pixel(const JpegDecodeArgs& a, long long p, int& file) {
    while (file + 1 < a.n && a.offsets[file + 1] <= p) ++file;                  // (a file has a pixel at least: at most a step per pixel of a dword)
    const int* f = a.files + (size_t)file * MM_JPEG_DEC_FILE_INTS;
    const int H = f[JD_H], W = f[JD_W], hd = (H + 1) / 2, wd = (W + 1) / 2;
    const int rem = (int)(p - a.offsets[file]), y = rem / W, x = rem % W;
    const JpegPlanes pl = jpeg_decode_planes(a, f);
    switch (f[JD_LAYOUT]) {
        case MM_JPG_420: return jpeg_pixel_at<MM_JPG_420>(pl, hd, wd, y, x);
        case MM_JPG_422: return jpeg_pixel_at<MM_JPG_422>(pl, hd, wd, y, x);
        case MM_JPG_444: return jpeg_pixel_at<MM_JPG_444>(pl, hd, wd, y, x);
        default: {
            const unsigned v = *pl.luma(JpegMcu<MM_JPG_GREY>::W, y, x);
            return a.channels == 3 ? v * 0x010101u : v;
        }
    }
}

__global__ __launch_bounds__(MM_JPGD_BLOCK) void jpeg_decode_pixels_kernel(JpegDecodeArgs a) {
    const int lead = (int)((uintptr_t)a.out & 3);             // bytes of the first aligned dword that lie before the output
    const long long i = (long long)blockIdx.x * MM_JPGD_BLOCK + threadIdx.x;
    const long long b0 = 4 * i - lead, first = max(b0, 0LL), last = min(b0 + 4, a.total_bytes);      // this lane's bytes [first, last)
    if (first >= last) return;
    const long long p = first / a.channels;
    int lo = 0, hi = a.n - 1;                                 // the file of pixel p: the last whose offset is <= p
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.offsets[mid] <= p) lo = mid; else hi = mid - 1;
    }
    unsigned w = 0;
    if (a.channels == 3) w = jpeg_rgb_bytes(first, last, [&](long long q) { return jpeg_decode_pixel(a, q, lo); });
    else for (long long b = first; b < last; ++b) w |= jpeg_decode_pixel(a, b, lo) << (8 * (int)(b - first));
    jpeg_store_bytes(a.out, first, last, w);                  // (a whole dword: first = b0, and out + b0 is a multiple of 4)
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
int launch_jpeg_decode(const MMJpegDecodeDesc* d, hipStream_t s) {
    const JpegDecodeTables t = jpeg_decode_tables(d);
    const JpegDecodeLayout l = jpeg_decode_layout(d);
    const JpegDecodeTotals r = jpeg_decode_totals(d);
    unsigned char* ws = (unsigned char*)d->workspace;
    JpegDecodeArgs a = {};
    a.bytes = d->bytes;
    a.files = d->tables + t.files; a.offsets = (const long long*)(d->tables + t.offsets); a.segments = d->tables + t.segments;
    a.qtables = d->tables + t.qtables; a.htables = (const unsigned*)(d->tables + t.htables); a.sets = d->tables + t.sets;
    a.coef = (short*)(ws + l.coef); a.status = (int*)(ws + l.status); a.planes = ws + l.planes; a.out = d->out;
    a.n = d->n; a.channels = d->mode == MM_JPEG_MODE_RGB ? 3 : 1;
    a.total_blocks = r.blocks; a.total_bytes = r.pixels * a.channels;
    if (hipMemsetAsync(ws + l.coef, 0, l.planes - l.coef, s) != hipSuccess) return launch_ok("jpeg_decode_zero");      // coefficients and status
    hipLaunchKernelGGL(jpeg_decode_entropy_kernel, dim3((unsigned)(d->n_segments / MM_JPEG_DEC_GROUP)), dim3(MM_JPGD_WAVE), 0, s, a);
    hipLaunchKernelGGL(jpeg_decode_idct_kernel, dim3((unsigned)((a.total_blocks + MM_JPGD_BLOCK / 8 - 1) / (MM_JPGD_BLOCK / 8))), dim3(MM_JPGD_BLOCK), 0, s, a);
    const long long dwords = (a.total_bytes + 3 + 3) / 4;     // the aligned dwords the output touches, at most
    hipLaunchKernelGGL(jpeg_decode_pixels_kernel, dim3((unsigned)((dwords + MM_JPGD_BLOCK - 1) / MM_JPGD_BLOCK)), dim3(MM_JPGD_BLOCK), 0, s, a);
    return launch_ok("jpeg_decode");
}

}  // namespace mm
