// mm_png_decode.hip -- PNG FILES to 8-bit device frames, for gfx950: what the reference's seg_loaders do on the host per file with
// Image.open(f).convert('L') (datasets/bird.py, atr.py, market.py) or .convert('RGBA') (datasets/thuman2.py), and what reads this project's
// own encode_png files back.  The caller walks the chunks (png_decode.py: lower_png_decode); the tables it hands over are described at
// MMPngDecodeDesc in include/mm_render.h, and every record is re-checked here, on the host, before anything is launched (check_png_decode).
//
// One memset (the inflated streams and the status words, adjacent in the workspace) and three launches, whatever the number of files:
//   inflate   one wave per file (a workgroup is one wave).  The symbol chain is decoded uniformly across the wave; the lanes share the rest:
//             the input window, the code tables in LDS, stored-block and match copies.  mm_inflate.h has the text and THE LOOP-BOUND
//             INVARIANT: every loop trip consumes an input bit or produces an output byte, consumed bits are capped by the record's byte range
//             (the first bit wanted past it ends the decode) and produced bytes by the record's S = H * (1 + row_bytes), so no byte sequence
//             makes the kernel spin, or read outside [begin, end) of its file or write outside its S bytes.  Back-references read S from
//             the workspace.
//   unfilter  one wave per file, in place in S, a band of 64 rows at a time as a skewed wavefront: lane r takes row r of the band and at step
//             t byte t - r, so "up" is lane r - 1's value of the step before, "up-left" that lane's value bpp steps earlier (one cross-lane
//             shift carries both), "left" the lane's own value bpp steps back -- a band costs row_bytes + 63 steps.  Lane 0 reads the row
//             above the band from memory.  The arithmetic is mod 256: any schedule gives these bytes.  A filter byte above 4 sets
//             MM_PNG_ST_BAD_FILTER and the row is taken as filter 0.
//   pixels    one lane per aligned dword of the output, whatever byte `out` starts at: per byte its pixel, the pixel's file by bisection of
//             the pixel offsets, the sample(s) out of S (1/2/4-bit samples unpacked, high bits first), through the file's conversion table
//             (grey and palette files) or the direct rule (grey+alpha, RGB, RGBA), one 4-byte store -- byte stores at the output's two ends.
// No floating point, no atomics but the OR into a file's status word, no scratch; every output byte is a pure function of the files.
#include <hip/hip_runtime.h>

#include <cstring>

#include "mm_device.h"
#include "mm_inflate.h"
#include "mm_jpeg_idct.h"                                     // jpeg_store_bytes
#include "mm_stream.h"                                        // Carve

#define MM_PNGD_BLOCK 256
#define MM_PNGD_WAVE 64

namespace mm {

// the words of a file record
enum { PD_H = 0, PD_W = 1, PD_CTYPE = 2, PD_DEPTH = 3, PD_BPP = 4, PD_ROWB = 5, PD_TABLE = 6, PD_BEGIN = 7, PD_END = 8, PD_SOFF = 9 };

__host__ __device__ inline int png_channels_in(int ctype) { return ctype == 2 ? 3 : ctype == 4 ? 2 : ctype == 6 ? 4 : 1; }

struct PngDecodeTables { size_t files, offsets, conv, words; };          // where the tables lie in MMPngDecodeDesc.tables (32-bit words)
__host__ PngDecodeTables png_decode_tables(const MMPngDecodeDesc* d) {
    PngDecodeTables t;
    t.files = 0;
    t.offsets = t.files + (size_t)d->n * MM_PNG_DEC_FILE_INTS;
    t.conv = t.offsets + 2 * ((size_t)d->n + 1);
    t.words = t.conv + (size_t)d->n_tables * 256;
    return t;
}

struct PngDecodeLayout { size_t streams, status, bytes; long long stream_bytes, pixels; };
__host__ PngDecodeLayout png_decode_layout(const MMPngDecodeDesc* d) {   // of a call whose records passed check_png_decode
    const PngDecodeTables t = png_decode_tables(d);
    const int32_t* f = d->tables_host + t.files + (size_t)(d->n - 1) * MM_PNG_DEC_FILE_INTS;
    PngDecodeLayout l;
    l.stream_bytes = f[PD_SOFF] + (long long)f[PD_H] * (1 + f[PD_ROWB]);
    std::memcpy(&l.pixels, d->tables_host + t.offsets + 2 * (size_t)d->n, 8);
    Carve c;
    l.streams = c.take((size_t)l.stream_bytes);
    l.status = c.take((size_t)d->n * 4);
    l.bytes = c.at;
    return l;
}
size_t png_decode_workspace_bytes(const MMPngDecodeDesc* d) { return png_decode_layout(d).bytes; }

// Every record of tables_host, before anything is launched: the kernels index with what these records say and with nothing else.
int check_png_decode(const MMPngDecodeDesc* d) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->n < 1 || d->n_tables < 0 || d->n_bytes < 1) return MM_ERR_BAD_SHAPE;
    if (d->channels != 1 && d->channels != 3 && d->channels != 4) return MM_ERR_BAD_SHAPE;
    if (d->post < 0 || d->post > 3 || ((d->post & MM_PNG_POST_ALPHA) && d->channels != 4)) return MM_ERR_BAD_SHAPE;
    if (d->n > MM_PNG_DEC_MAX_FILES || d->n_bytes > MM_PNG_DEC_MAX_BYTES) return MM_ERR_UNSUPPORTED;
    if (!d->tables_host) return MM_ERR_NULL_POINTER;
    const PngDecodeTables t = png_decode_tables(d);
    const int32_t* tab = d->tables_host;
    long long soff = 0, pixel = 0;
    for (int i = 0; i < d->n; ++i) {
        const int32_t* f = tab + t.files + (size_t)i * MM_PNG_DEC_FILE_INTS;
        const int H = f[PD_H], W = f[PD_W], ct = f[PD_CTYPE], dp = f[PD_DEPTH];
        if (H < 1 || W < 1) return MM_ERR_BAD_SHAPE;
        if (H > 65535 || W > 65535) return MM_ERR_UNSUPPORTED;
        if (ct != 0 && ct != 2 && ct != 3 && ct != 4 && ct != 6) return MM_ERR_BAD_SHAPE;
        if (dp == 16) return MM_ERR_UNSUPPORTED;
        if (dp != 8 && !((ct == 0 || ct == 3) && (dp == 1 || dp == 2 || dp == 4))) return MM_ERR_BAD_SHAPE;
        const int cin = png_channels_in(ct);
        if (f[PD_BPP] != (dp < 8 ? 1 : cin) || f[PD_ROWB] != (int)(((long long)W * cin * dp + 7) / 8)) return MM_ERR_BAD_SHAPE;
        if (ct == 0 || ct == 3) { if (f[PD_TABLE] < 0 || f[PD_TABLE] >= d->n_tables) return MM_ERR_BAD_SHAPE; }
        else if (f[PD_TABLE] != -1) return MM_ERR_BAD_SHAPE;
        if (f[PD_BEGIN] < 0 || f[PD_END] < f[PD_BEGIN] || f[PD_END] > d->n_bytes) return MM_ERR_BAD_SHAPE;
        if (f[PD_SOFF] != soff) return MM_ERR_BAD_SHAPE;
        soff += (long long)H * (1 + f[PD_ROWB]);
        if (soff > MM_PNG_DEC_MAX_BYTES) return MM_ERR_UNSUPPORTED;
        long long at, next;
        std::memcpy(&at, tab + t.offsets + 2 * (size_t)i, 8);
        std::memcpy(&next, tab + t.offsets + 2 * (size_t)i + 2, 8);
        if (at != pixel || next != pixel + (long long)H * W) return MM_ERR_BAD_SHAPE;
        pixel = next;
        if (pixel > MM_PNG_DEC_MAX_PIXELS) return MM_ERR_UNSUPPORTED;
    }
    return MM_OK;
}

struct PngDecodeArgs {
    const unsigned char* bytes;
    const int* files; const long long* offsets; const unsigned* conv;
    unsigned char* streams; int* status; unsigned char* out;
    int n, cmode, channels, post;                             // cmode: the conversion's channels; channels: bytes a pixel of out
    long long total_bytes;
};

// ---- inflate: a file's IDAT data -> its filtered stream S -------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_PNGD_WAVE) void png_inflate_kernel(PngDecodeArgs a) {
    __shared__ InfShared sh;
    const int* f = a.files + (size_t)blockIdx.x * MM_PNG_DEC_FILE_INTS;
    const int S = f[PD_H] * (1 + f[PD_ROWB]);
    const int st = inflate_stream(a.bytes, f[PD_BEGIN], f[PD_END], a.streams + (size_t)f[PD_SOFF], S, &sh);
    if (st && threadIdx.x == 0) atomicOr(a.status + blockIdx.x, st);
}

// ---- unfilter: S in place --------------------------------------------------------------------------------------------------------------
__device__ inline int png_paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

__global__ __launch_bounds__(MM_PNGD_WAVE) void png_unfilter_kernel(PngDecodeArgs a) {
    const int* f = a.files + (size_t)blockIdx.x * MM_PNG_DEC_FILE_INTS;
    const int H = f[PD_H], rb = f[PD_ROWB], bpp = f[PD_BPP], lane = threadIdx.x;
    unsigned char* S = a.streams + (size_t)f[PD_SOFF];
    const size_t pitch = (size_t)rb + 1;
    bool bad = false;
    for (int y0 = 0; y0 < H; y0 += MM_PNGD_WAVE) {
        __syncthreads();                                      // the band above is written (one wave: no more than a fence)
        const int y = y0 + lane;
        const bool row = y < H;
        unsigned char* cur = S + (size_t)(row ? y : 0) * pitch;
        const unsigned char* above = lane == 0 && y0 > 0 ? S + (size_t)(y0 - 1) * pitch + 1 : nullptr;      // lane 0's row above, from memory
        int ft = row ? cur[0] : 0;
        if (ft > 4) { bad = true; ft = 0; }
        unsigned long long hist = 0, uhist = 0;               // byte k: this row's (lane 0: the row above's) byte x - 1 - k
        for (int t = 0; t < rb + MM_PNGD_WAVE - 1; ++t) {
            const unsigned mine = (unsigned)(hist & 0xFF) | (unsigned)((hist >> (8 * bpp)) & 0xFF) << 8;      // byte x' and byte x' - bpp of this row, x' = t - 1 - lane
            unsigned up2 = (unsigned)__shfl_up((int)mine, 1, MM_PNGD_WAVE);
            const int x = t - lane;
            if (lane == 0) {
                const unsigned u = above && x < rb ? above[x] : 0u;
                up2 = u | (unsigned)((uhist >> (8 * (bpp - 1))) & 0xFF) << 8;
                uhist = uhist << 8 | u;
            }
            if (row && x >= 0 && x < rb) {
                const int raw = cur[1 + x], left = (int)((hist >> (8 * (bpp - 1))) & 0xFF), up = (int)(up2 & 0xFF), ul = (int)(up2 >> 8 & 0xFF);
                const int pred = ft == 1 ? left : ft == 2 ? up : ft == 3 ? (left + up) >> 1 : ft == 4 ? png_paeth(left, up, ul) : 0;
                const unsigned v = (unsigned)(raw + pred) & 0xFF;
                cur[1 + x] = (unsigned char)v;
                hist = hist << 8 | v;
            }
        }
    }
    if (__ballot(bad) && lane == 0) atomicOr(a.status + blockIdx.x, MM_PNG_ST_BAD_FILTER);
}

// ---- pixels: unpack, convert, store -----------------------------------------------------------------------------------------------------
// Pillow's ImagingConvert L from RGB
__device__ inline unsigned png_luma(unsigned r, unsigned g, unsigned b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }

// pixel p of the output (its file is `file` or a later one; `file` is moved on to it): output channel c in byte c
__device__ inline unsigned png_decode_pixel(const PngDecodeArgs& a, long long p, int& file) {
    while (file + 1 < a.n && a.offsets[file + 1] <= p) ++file;                  // (a file has a pixel at least)
    const int* f = a.files + (size_t)file * MM_PNG_DEC_FILE_INTS;
    const int W = f[PD_W], ct = f[PD_CTYPE], dp = f[PD_DEPTH];
    const long long rem = p - a.offsets[file];
    const int y = (int)(rem / W), x = (int)(rem % W);
    const unsigned char* row = a.streams + (size_t)f[PD_SOFF] + (size_t)y * ((size_t)f[PD_ROWB] + 1) + 1;
    if (ct == 0 || ct == 3) {
        const int bit = x * dp;
        const unsigned v = (row[bit >> 3] >> (8 - dp - (bit & 7))) & ((1u << dp) - 1u);
        return a.conv[(size_t)f[PD_TABLE] * 256 + v];
    }
    if (ct == 4) {
        const unsigned g = row[2 * x], al = row[2 * x + 1];
        return a.cmode == 1 ? g : g * 0x010101u | al << 24;
    }
    const int cin = ct == 2 ? 3 : 4;
    const unsigned r = row[cin * x], g = row[cin * x + 1], b = row[cin * x + 2], al = ct == 6 ? row[4 * x + 3] : 255u;
    return a.cmode == 1 ? png_luma(r, g, b) : r | g << 8 | b << 16 | al << 24;
}
// ... and what MMPngDecodeDesc.post makes of it: the alpha plane alone, every byte that is not 0 as 255
__device__ inline unsigned png_post_pixel(const PngDecodeArgs& a, long long p, int& file) {
    unsigned e = png_decode_pixel(a, p, file);
    if (a.post & MM_PNG_POST_ALPHA) e >>= 24;
    if (a.post & MM_PNG_POST_THRESHOLD) e = (e & 0xFFu ? 0xFFu : 0u) | (e & 0xFF00u ? 0xFF00u : 0u) | (e & 0xFF0000u ? 0xFF0000u : 0u) | (e & 0xFF000000u ? 0xFF000000u : 0u);
    return e;
}

__global__ __launch_bounds__(MM_PNGD_BLOCK) void png_pixels_kernel(PngDecodeArgs a) {
    const int lead = (int)((uintptr_t)a.out & 3);             // bytes of the first aligned dword that lie before the output
    const long long i = (long long)blockIdx.x * MM_PNGD_BLOCK + threadIdx.x;
    const long long b0 = 4 * i - lead, first = max(b0, 0LL), last = min(b0 + 4, a.total_bytes);      // this lane's bytes [first, last)
    if (first >= last) return;
    long long p = first / a.channels;
    int lo = 0, hi = a.n - 1;                                 // the file of pixel p: the last whose offset is <= p
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.offsets[mid] <= p) lo = mid; else hi = mid - 1;
    }
    unsigned e = png_post_pixel(a, p, lo), w = 0;
    for (long long b = first; b < last; ++b) {
        const long long q = b / a.channels;
        if (q != p) { p = q; e = png_post_pixel(a, p, lo); }
        w |= ((e >> (8 * (int)(b - q * a.channels))) & 0xFFu) << (8 * (int)(b - first));
    }
    jpeg_store_bytes(a.out, first, last, w);                  // (a whole dword: first = b0, and out + b0 is a multiple of 4)
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
int launch_png_decode(const MMPngDecodeDesc* d, hipStream_t s) {
    const PngDecodeTables t = png_decode_tables(d);
    const PngDecodeLayout l = png_decode_layout(d);
    unsigned char* ws = (unsigned char*)d->workspace;
    PngDecodeArgs a = {};
    a.bytes = d->bytes;
    a.files = d->tables + t.files; a.offsets = (const long long*)(d->tables + t.offsets); a.conv = (const unsigned*)(d->tables + t.conv);
    a.streams = ws + l.streams; a.status = (int*)(ws + l.status); a.out = d->out;
    a.n = d->n; a.cmode = d->channels; a.channels = (d->post & MM_PNG_POST_ALPHA) ? 1 : d->channels; a.post = d->post;
    a.total_bytes = l.pixels * a.channels;
    if (hipMemsetAsync(ws + l.streams, 0, l.bytes - l.streams, s) != hipSuccess) return launch_ok("png_decode_zero");      // the streams and the status words
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)d->n), dim3(MM_PNGD_WAVE), 0, s, a);
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)d->n), dim3(MM_PNGD_WAVE), 0, s, a);
    const long long dwords = (a.total_bytes + 3 + 3) / 4;     // the aligned dwords the output touches, at most
    hipLaunchKernelGGL(png_pixels_kernel, dim3((unsigned)((dwords + MM_PNGD_BLOCK - 1) / MM_PNGD_BLOCK)), dim3(MM_PNGD_BLOCK), 0, s, a);
    return launch_ok("png_decode");
}

}  // namespace mm
