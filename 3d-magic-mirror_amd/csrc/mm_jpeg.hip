// mm_jpeg.hip -- 8-bit device frames (n,H,W,3) as baseline JPEG files, for gfx950: what the reference's scripts do on the host per image with
// to_pil_image(X[i, :3].cpu()).save(name, 'JPEG', quality=100) (trainer.py:51, test.py:53, generate_market++.py:55,
// tool/generate_market_test.py:57, ...).  Every file equals Pillow's (libjpeg-turbo's) byte for byte: baseline, 4:2:0, the standard
// Huffman tables.  The MCU is a template parameter (JpegMcu of mm_jpeg_idct.h): 4:2:0 is written out here; 4:2:2, 4:4:4 and greyscale -- masks (n,H,W),
// the files to_pil_image(X[i, 3]).save(...) writes -- differ in the edges, the chroma and the block order alone, as said at JpegMcu.  The host makes the tables and the header; everything after SOS is made here.  Integer arithmetic only (>> is
// arithmetic), in libjpeg's order:
//   colour    Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
//             Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//             Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
//   edges     an MCU is 16 x 16 pixels: four luma blocks Y00 Y01 Y10 Y11 and one block each of Cb and Cr.  Columns beyond W replicate the
//             INPUT's last column; rows beyond H replicate the input's last row up to an even height; the chroma rows beyond ceil(H / 2)
//             replicate the DOWNSAMPLED last row (this differs from replicating input rows when H is even and H mod 16 is in 1..8).
//             A luma block wholly beyond ceil(W / 8) or ceil(H / 8) is a DUMMY: no AC, and the DC of the block before it in MCU order.
//   chroma    c[y][x] = (C[2y][2x] + C[2y][2x+1] + C[2y+1][2x] + C[2y+1][2x+1] + bias) >> 2, bias 1 on even x and 2 on odd x
//   DCT       jfdctint's islow transform of the samples minus 128: CONST_BITS 13, PASS1_BITS 2, rows first, then columns; scaled by 8
//   quantise  q = sign(v) * ((|v| + (d >> 1)) / d), d = 8 * table[k]: half away from zero
//   entropy   MCUs in raster order, blocks Y00 Y01 Y10 Y11 Cb Cr, one DC predictor per component; the DC difference and every non-zero AC
//             as (code of run << 4 | category, then category bits of v, or of v - 1 below zero); sixteen zeros as ZRL (0xF0); EOB unless the
//             last coefficient is non-zero; the last byte padded with 1-bits; a 0x00 after every 0xFF; EOI.
//
// Eight launches and one memset, all on the caller's stream, nothing synchronises:
//   transform eight lanes per block.  Lane r loads row r of its block (luma: 8 pixels; chroma: 16 x 2 pixels, converted and downsampled),
//             runs the row pass, the block is transposed through LDS, lane c runs the column pass and quantises, and the block leaves as
//             int16 in zigzag order, 16 bytes per lane.  The edges are clamped indices: nothing is padded in memory.
//   count     one lane per block walks its 64 coefficients and writes the block's exact bit count.  The DC difference needs the previous
//             block of the same component only, which is in memory already: no lane waits for another.
//   offsets   one workgroup per frame scans the counts in MCU order: every block's bit offset, the frame's bits.  (This scan, place's and
//             files' are array_scan of mm_stream.h, the loop the GIF encoder's scans share: 256 elements a pass behind a running carry.)
//   pack      one lane per block walks again and ORs its codes into the frame's zeroed stream, big-endian 32-bit words.  Only a block's
//             first and last word are shared with its neighbours (atomic OR, integer: the result is the same in any order), the words
//             between them are stored plainly.
//   count FF  a workgroup per 1024-byte chunk of a stream counts its 0xFF bytes; the lane that holds the last byte pads it with 1-bits.
//   place     one workgroup per frame scans its chunks' counts; the frame's length is header + bytes + stuffed + 2.
//   files     one workgroup scans the lengths: offsets[0..n], the files lie back to back.
//   write     a workgroup per chunk scans its lanes' counts and writes the stuffed bytes where they go; chunk 0 also writes the
//             header, the lane with the last byte also EOI.
// A stream is never assumed to fit LDS (256 x 256 noise at quality 100 is 130 KB): it lives in the workspace, MM_JPEG_BLOCK_BYTES = 208 per
// block (a block codes to 20 + 63 * 26 bits at most), and a file's room is header + twice that + 2.  No floating point, no scratch; every
// byte is a pure function of the frame (bitwise reproducible).
// The round trip (mm_jpeg_roundtrip: the frames as the decoder reads those files back) is below the encoder's kernels, with its own header.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "mm_device.h"
#include "mm_jpeg_idct.h"                                    // JpegMcu and the decoder's back half: shared with mm_jpeg_decode.hip
#include "mm_quant.h"                                         // unquant: the v / 255 of as_float, shared with the exports
#include "mm_stream.h"                                        // array_scan, Carve: what the encoders share

#define MM_JPG_BLOCK 256
#define MM_JPG_BLOCK_WORDS (MM_JPEG_BLOCK_BYTES / 4)
#define MM_JPG_CHUNK_WORDS (MM_JPEG_CHUNK_BYTES / 4)
static_assert(MM_JPG_CHUNK_WORDS == MM_JPG_BLOCK, "a lane per word of a chunk");

namespace mm {

// where the tables lie in MMJpegDesc.params (32-bit words)
enum { MM_JPG_DIV = 0, MM_JPG_HUFF = 128, MM_JPG_HEADER = 128 + 1024 };

// What an MCU is, said once.  A layout's number is its MM_JPEG_SAMPLING_* for colour (0: 4:2:0, 1: 4:2:2, 2: 4:4:4) and 3 for greyscale.
// The first LUMA blocks of an MCU are luma (or grey), LH across and LV down in raster order, and use the luma divisors and tables; in a
// colour layout one block each of Cb and Cr follows, with the chroma divisors and tables.  Colour, DCT, quantiser and entropy coder are
// the same in every layout; per layout:
//   4:2:0      16 x 16 pixels, Y00 Y01 Y10 Y11 Cb Cr: the header of this file.
//   4:2:2      16 wide, 8 high, Y0 Y1 Cb Cr.  Columns beyond W replicate the input's last column up to the MCU, rows beyond H its last row
//              up to the block.  c[x] = (C[2x] + C[2x+1] + bias) >> 1, bias 0 on even x and 1 on odd x.  Y1 is a dummy where
//              2 mx + 1 >= ceil(W / 8) (W mod 16 in 1..8).  No vertical dummy, no downsampled-row rule.
//   4:4:4      8 x 8 pixels, Y Cb Cr; edges replicated on all three planes; no downsampling, no dummies.
//   greyscale  a non-interleaved scan: an MCU is one 8 x 8 block, ceil(H / 8) x ceil(W / 8) in raster order, edges replicated, no dummies;
//              the frames are (n,H,W), one byte a pixel; the luma divisors and tables, one DC predictor.
// Decoding (the round trip below): the sample planes are Y 8 LV my x 8 LH mx and Cb, Cr 8 my x 8 mx per frame.  4:4:4 is not upsampled;
// 4:2:2 has real chroma on H x wd, wd = ceil(W / 2): wd > 2, h2v1 fancy, out[2x] = (3 s[x] + s[x-1] + 1) >> 2, out[2x+1] =
// (3 s[x] + s[x+1] + 2) >> 2, s[-1] := s[0], s[wd] := s[wd-1]; wd <= 2, replication; no vertical neighbour.
template <int N = 4, class F>
__host__ inline void jpeg_by_layout(int layout, F f) {       // f(std::integral_constant<int, layout>): the host's dispatch on the template parameter
    switch (layout) {
        case MM_JPG_420: f(std::integral_constant<int, MM_JPG_420>()); break;
        case MM_JPG_422: f(std::integral_constant<int, MM_JPG_422>()); break;
        case MM_JPG_444: f(std::integral_constant<int, MM_JPG_444>()); break;
        default: if constexpr (N > MM_JPG_GREY) f(std::integral_constant<int, MM_JPG_GREY>()); break;
    }
}
// mode and sampling as the descriptors carry them -> the layout, or -1 for what is refused (an unknown value; a sampling with mode L)
int jpeg_layout_of(int mode, int sampling) {
    if (mode == MM_JPEG_MODE_L) return sampling == 0 ? MM_JPG_GREY : -1;
    if (mode != MM_JPEG_MODE_RGB || sampling < MM_JPEG_SAMPLING_420 || sampling > MM_JPEG_SAMPLING_444) return -1;
    return sampling;
}
long long jpeg_frame_blocks(int H, int W, int layout) {
    const JpegMcuShape m = jpeg_mcu_shape(layout);
    return (long long)m.blocks * ((H + m.h - 1) / m.h) * ((W + m.w - 1) / m.w);
}

struct JpegLayout {
    int layout, my, mx, blocks, chunks;                       // MCU rows and columns, blocks and 1024-byte chunks of one frame
    size_t file_cap;                                          // bytes kept for one file
    size_t offsets, files, coef, bits, frame_bits, raw, chunk_ff, bytes;      // byte offsets into the workspace
};
__host__ JpegLayout jpeg_layout(const MMJpegModesDesc* d) {
    JpegLayout l;
    l.layout = jpeg_layout_of(d->mode, d->sampling);
    const JpegMcuShape m = jpeg_mcu_shape(l.layout);
    l.my = (d->H + m.h - 1) / m.h; l.mx = (d->W + m.w - 1) / m.w;
    l.blocks = l.my * l.mx * m.blocks;
    l.chunks = (int)(((size_t)l.blocks * MM_JPEG_BLOCK_BYTES + MM_JPEG_CHUNK_BYTES - 1) / MM_JPEG_CHUNK_BYTES);
    l.file_cap = (size_t)d->header_bytes + 2 * (size_t)l.chunks * MM_JPEG_CHUNK_BYTES + 2;
    const size_t n = (size_t)d->n;
    Carve c;
    l.offsets = c.take((n + 1) * 8);
    l.files = c.take(n * l.file_cap);
    l.coef = c.take(n * l.blocks * 128);
    l.bits = c.take(n * l.blocks * 4);
    l.frame_bits = c.take(n * 4);
    l.raw = c.take(n * l.chunks * MM_JPEG_CHUNK_BYTES);
    l.chunk_ff = c.take(n * l.chunks * 4);
    l.bytes = c.at;
    return l;
}
size_t jpeg_workspace_bytes(const MMJpegModesDesc* d) { return jpeg_layout(d).bytes; }
size_t jpeg_files_at(const MMJpegModesDesc* d) { return jpeg_layout(d).files; }

struct JpegArgs {
    const unsigned char* frames; const int* par;
    long long* offsets; unsigned char* files; short* coef; unsigned* bits; unsigned* frame_bits; unsigned* raw; unsigned* chunk_ff;
    int n, H, W, header_bytes;
    int my, mx, blocks, chunks;
    int bh, bw, ch;                                           // luma blocks down and across that hold pixels; 4:2:0: chroma rows that do
    long long total_blocks;
};

// ---- small pieces ------------------------------------------------------------------------------------------------------------------
// one pass of jfdctint over eight values; FIRST: the row pass (output scaled up by PASS1_BITS), else the column pass
template <bool FIRST>
__device__ inline void jpeg_fdct8(const int (&d)[8], int (&o)[8]) {
    constexpr int CB = 13, PB = 2;
    constexpr int N = FIRST ? CB - PB : CB + PB, R = 1 << (N - 1);
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) { o[0] = (t10 + t11) * (1 << PB); o[4] = (t10 - t11) * (1 << PB); }
    else       { o[0] = (t10 + t11 + (1 << (PB - 1))) >> PB; o[4] = (t10 - t11 + (1 << (PB - 1))) >> PB; }
    int z1 = (t12 + t13) * 4433;
    o[2] = (z1 + t13 * 6270 + R) >> N;
    o[6] = (z1 + t12 * -15137 + R) >> N;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    o[7] = (a4 + z1 + z3 + R) >> N;
    o[5] = (a5 + z2 + z4 + R) >> N;
    o[3] = (a6 + z2 + z3 + R) >> N;
    o[1] = (a7 + z1 + z4 + R) >> N;
}

// ---- transform: frames -> quantised coefficients, zigzag order, MCU order ---------------------------------------------------------
// Cb or Cr of one pixel
__device__ inline int jpeg_chroma(const unsigned char* p, bool cb) {
    const int R = p[0], G = p[1], B = p[2];
    return cb ? (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
              : (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
}

template <int L>
__global__ __launch_bounds__(MM_JPG_BLOCK) void jpeg_transform_kernel(JpegArgs a) {
    using M = JpegMcu<L>;
    __shared__ int tile[MM_JPG_BLOCK / 8][65];                // a block's 64 values after the row pass (65: the blocks' rows on different banks)
    __shared__ __attribute__((aligned(16))) short zz[MM_JPG_BLOCK / 8][64];
    const int tid = threadIdx.x, lb = tid >> 3, r = tid & 7;
    const long long g = (long long)blockIdx.x * (MM_JPG_BLOCK / 8) + lb;      // the block, over all frames
    const bool live = g < a.total_blocks;
    const long long gc = live ? g : 0;
    const int img = (int)(gc / a.blocks), rem = (int)(gc % a.blocks);
    const int mcu = rem / M::BLOCKS, j = rem % M::BLOCKS, my = mcu / a.mx, mx = mcu % a.mx;
    const unsigned char* f = a.frames + (size_t)img * a.H * a.W * M::CHANNELS;
    bool dummy = false;
    int d[8], o[8];
    if (j < M::LUMA) {
        const int by = M::LV * my + (j >> M::LH_SHIFT), bx = M::LH * mx + (j & (M::LH - 1));
        dummy = by >= a.bh || bx >= a.bw;
        const int y = min(by * 8 + r, a.H - 1);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const unsigned char* p = f + ((size_t)y * a.W + min(bx * 8 + c, a.W - 1)) * M::CHANNELS;
            if constexpr (L == MM_JPG_GREY) d[c] = (int)p[0] - 128;
            else d[c] = ((19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16) - 128;
        }
    } else if constexpr (L == MM_JPG_444) {                   // chroma as it is
        const size_t y = (size_t)min(my * 8 + r, a.H - 1) * a.W;
#pragma unroll
        for (int c = 0; c < 8; ++c) d[c] = jpeg_chroma(f + (y + min(mx * 8 + c, a.W - 1)) * 3, j == M::LUMA) - 128;
    } else if constexpr (L == MM_JPG_422) {                   // 16 pixels of one row, halved across
        const size_t y = (size_t)min(my * 8 + r, a.H - 1) * a.W;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int x0 = min(2 * (mx * 8 + c), a.W - 1), x1 = min(2 * (mx * 8 + c) + 1, a.W - 1);
            const int sum = (c & 1) + jpeg_chroma(f + (y + x0) * 3, j == M::LUMA) + jpeg_chroma(f + (y + x1) * 3, j == M::LUMA);   // bias 0 on even output columns, 1 on odd ones
            d[c] = (sum >> 1) - 128;
        }
    } else if constexpr (L == MM_JPG_420) {
        const int cy = min(my * 8 + r, a.ch - 1);             // beyond the chroma rows: the downsampled last row
        const size_t y0 = (size_t)min(2 * cy, a.H - 1) * a.W, y1 = (size_t)min(2 * cy + 1, a.H - 1) * a.W;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int x0 = min(2 * (mx * 8 + c), a.W - 1), x1 = min(2 * (mx * 8 + c) + 1, a.W - 1);
            const unsigned char* q[4] = {f + (y0 + x0) * 3, f + (y0 + x1) * 3, f + (y1 + x0) * 3, f + (y1 + x1) * 3};
            int sum = (c & 1) + 1;                            // the bias: 1 on even output columns, 2 on odd ones
#pragma unroll
            for (int i = 0; i < 4; ++i) sum += jpeg_chroma(q[i], j == M::LUMA);
            d[c] = (sum >> 2) - 128;
        }
    }
    jpeg_fdct8<true>(d, o);
#pragma unroll
    for (int c = 0; c < 8; ++c) tile[lb][r * 8 + c] = o[c];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = tile[lb][k * 8 + r];   // lane r now has column r
    jpeg_fdct8<false>(d, o);
    const int* div = a.par + MM_JPG_DIV + (j < M::LUMA ? 0 : 64);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int nat = k * 8 + r;
        const unsigned dv = (unsigned)div[nat];
        const int v = o[k];
        const unsigned m = ((unsigned)abs(v) + (dv >> 1)) / dv;
        zz[lb][jpeg_zigzag_pos[nat]] = dummy ? (short)0 : (short)(v < 0 ? -(int)m : (int)m);
    }
    __syncthreads();
    if (live) *(uint4*)(a.coef + (size_t)g * 64 + r * 8) = *(const uint4*)&zz[lb][r * 8];
}

// ---- the walk over a block, shared by the count and the pack ----------------------------------------------------------------------
template <int L>
__device__ inline bool jpeg_is_dummy(const JpegArgs& a, int mcu, int j) {
    using M = JpegMcu<L>;
    if constexpr (M::LUMA == 1) return false;                 // one luma block an MCU: it always holds pixels
    return j < M::LUMA && (M::LV * (mcu / a.mx) + (j >> M::LH_SHIFT) >= a.bh || M::LH * (mcu % a.mx) + (j & (M::LH - 1)) >= a.bw);
}
// the DC a block codes: its own, or for a dummy that of the block before it in MCU order (an MCU's first block is never a dummy)
template <int L>
__device__ inline int jpeg_dc(const JpegArgs& a, const short* frame_coef, int mcu, int j) {
    while (jpeg_is_dummy<L>(a, mcu, j)) --j;
    return frame_coef[((size_t)mcu * JpegMcu<L>::BLOCKS + j) * 64];
}
// the predictor: the DC coded by the previous block of the same component
template <int L>
__device__ inline int jpeg_dc_pred(const JpegArgs& a, const short* frame_coef, int mcu, int j) {
    if (j >= 1 && j < JpegMcu<L>::LUMA) return jpeg_dc<L>(a, frame_coef, mcu, j - 1);
    if (mcu == 0) return 0;
    return jpeg_dc<L>(a, frame_coef, mcu - 1, j == 0 ? JpegMcu<L>::LUMA - 1 : j);
}

struct JpegCounter {
    unsigned nbits = 0;
    __device__ inline void put(unsigned, int len) { nbits += len; }
    __device__ inline void finish() {}
};
// bits go out most significant first, into big-endian 32-bit words that were zeroed
struct JpegWriter {
    unsigned* word; unsigned* end;
    unsigned long long acc = 0;
    int nacc;                                                 // bits in acc, the first word's earlier bits (other blocks') as zeros
    bool first = true;
    __device__ inline JpegWriter(unsigned* w, unsigned* e, int used) : word(w), end(e), nacc(used) {}
    __device__ inline void put(unsigned v, int len) {         // len <= 27
        acc = (acc << len) | v;
        nacc += len;
        if (nacc >= 32) {
            nacc -= 32;
            const unsigned out = (unsigned)(acc >> nacc);
            if (word < end) { if (first) atomicOr(word, out); else *word = out; }
            first = false;
            ++word;
            acc &= (1ull << nacc) - 1;
        }
    }
    __device__ inline void finish() { if (nacc > 0 && word < end) atomicOr(word, (unsigned)(acc << (32 - nacc))); }
};

__device__ inline void jpeg_symbol(unsigned entry, int v, int cat, unsigned& bits, int& len) {
    const unsigned extra = (unsigned)(v < 0 ? v - 1 : v) & ((1u << cat) - 1);
    bits = ((entry & 0xFFFFu) << cat) | extra;
    len = (int)(entry >> 16) + cat;
}

// huff: the four tables in LDS (DC luma, AC luma, DC chroma, AC chroma), size << 16 | code per symbol
template <class Sink>
__device__ inline void jpeg_walk(const uint4* coef, int dc, int pred, const unsigned* dc_tab, const unsigned* ac_tab, Sink& sink) {
    unsigned bits; int len;
    {
        const int diff = dc - pred, cat = 32 - __clz(abs(diff));
        jpeg_symbol(dc_tab[cat], diff, cat, bits, len);
        sink.put(bits, len);
    }
    int run = 0;
    for (int g8 = 0; g8 < 8; ++g8) {
        const uint4 q = coef[g8];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (g8 == 0 && i == 0) continue;                  // the DC
            const int v = (int)(short)(w[i >> 1] >> (16 * (i & 1)));
            if (v == 0) { ++run; continue; }
            while (run > 15) { const unsigned z = ac_tab[0xF0]; sink.put(z & 0xFFFFu, (int)(z >> 16)); run -= 16; }
            // |v| < 1024 for 8-bit samples (libjpeg refuses more), so cat <= 10.  A category 11 would read a table entry of size 0 and make a
            // malformed stream, never an access outside the tables or the block's room (11 bits < 26).
            const int cat = 32 - __clz(abs(v));
            jpeg_symbol(ac_tab[((run << 4) | cat) & 0xFF], v, cat, bits, len);
            sink.put(bits, len);
            run = 0;
        }
    }
    if (run > 0) { const unsigned z = ac_tab[0]; sink.put(z & 0xFFFFu, (int)(z >> 16)); }
    sink.finish();
}

template <int L, bool PACK>
__global__ __launch_bounds__(MM_JPG_BLOCK) void jpeg_code_kernel(JpegArgs a) {
    using M = JpegMcu<L>;
    __shared__ unsigned huff[1024];
    const int tid = threadIdx.x;
    for (int i = tid; i < 1024; i += MM_JPG_BLOCK) huff[i] = (unsigned)a.par[MM_JPG_HUFF + i];
    __syncthreads();
    const long long g = (long long)blockIdx.x * MM_JPG_BLOCK + tid;
    if (g >= a.total_blocks) return;
    const int img = (int)(g / a.blocks), rem = (int)(g % a.blocks), mcu = rem / M::BLOCKS, j = rem % M::BLOCKS;
    const short* fc = a.coef + (size_t)img * a.blocks * 64;
    const int dc = jpeg_dc<L>(a, fc, mcu, j), pred = jpeg_dc_pred<L>(a, fc, mcu, j);
    const unsigned* dc_tab = huff + (j < M::LUMA ? 0 : 512);
    const uint4* coef = (const uint4*)(a.coef + (size_t)g * 64);
    if (PACK) {
        const unsigned at = a.bits[g];                        // the block's bit offset in its frame's stream
        unsigned* raw = a.raw + (size_t)img * a.chunks * MM_JPG_CHUNK_WORDS;
        JpegWriter w(raw + (at >> 5), raw + (size_t)a.chunks * MM_JPG_CHUNK_WORDS, (int)(at & 31));
        jpeg_walk(coef, dc, pred, dc_tab, dc_tab + 256, w);
    } else {
        JpegCounter c;
        jpeg_walk(coef, dc, pred, dc_tab, dc_tab + 256, c);
        a.bits[g] = c.nbits;
    }
}

// ---- offsets: per frame, the blocks' bit counts -> bit offsets, in place ------------------------------------------------------------
__global__ __launch_bounds__(MM_JPG_BLOCK) void jpeg_bit_offsets_kernel(JpegArgs a) {
    __shared__ unsigned sh[block_scan_words<MM_JPG_BLOCK, unsigned>()];
    const int tid = threadIdx.x, img = blockIdx.x;
    const unsigned carry = array_scan<false, MM_JPG_BLOCK>(a.bits + (size_t)img * a.blocks, a.blocks, 0u, tid, sh);
    // (a block of valid tables codes to 64 * 26 bits at most, so the sum fits; the clamp keeps every later index inside the frame's room whatever the tables)
    if (tid == 0) a.frame_bits[img] = min(carry, (unsigned)a.chunks * (MM_JPEG_CHUNK_BYTES * 8u));
}

// byte k of a stream lies in word k / 4 at shift 24 - 8 * (k % 4)
__device__ inline int jpeg_count_ff(unsigned w, int nbytes) {  // among the first nbytes (0..4) bytes of the word
    int c = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) c += (i < nbytes && ((w >> (24 - 8 * i)) & 0xFFu) == 0xFFu) ? 1 : 0;
    return c;
}

// ---- count FF: per chunk of a stream; pads the last byte --------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_JPG_BLOCK) void jpeg_count_ff_kernel(JpegArgs a) {
    __shared__ int sh[4];
    const int tid = threadIdx.x, chunk = blockIdx.x, img = blockIdx.y;
    const unsigned nbits = a.frame_bits[img];
    const long long len = ((long long)nbits + 7) >> 3;        // the stream's bytes
    const long long byte0 = (long long)chunk * MM_JPEG_CHUNK_BYTES + tid * 4;
    int c = 0;
    if (byte0 < len) {
        unsigned* p = a.raw + ((size_t)img * a.chunks + chunk) * MM_JPG_CHUNK_WORDS + tid;
        unsigned w = *p;
        const int nb = (int)min(len - byte0, 4LL);
        if (byte0 + nb == len && (nbits & 7)) {               // the last byte: its unused low bits become 1
            w |= (0xFFu >> (nbits & 7)) << (24 - 8 * (nb - 1));
            *p = w;
        }
        c = jpeg_count_ff(w, nb);
    }
    int total;
    (void)block_prefix_excl<MM_JPG_BLOCK>(c, tid, sh, total);
    if (tid == 0) a.chunk_ff[(size_t)img * a.chunks + chunk] = (unsigned)total;
}

// ---- place: per frame, the chunks' counts -> the stuffed bytes before each chunk, in place; the file's length -----------------------------
__global__ __launch_bounds__(MM_JPG_BLOCK) void jpeg_place_kernel(JpegArgs a) {
    __shared__ unsigned sh[block_scan_words<MM_JPG_BLOCK, unsigned>()];
    const int tid = threadIdx.x, img = blockIdx.x;
    const unsigned carry = array_scan<false, MM_JPG_BLOCK>(a.chunk_ff + (size_t)img * a.chunks, a.chunks, 0u, tid, sh);
    if (tid == 0) a.offsets[img + 1] = (long long)a.header_bytes + (((long long)a.frame_bits[img] + 7) >> 3) + carry + 2;
}

// ---- files: the lengths in offsets[1..n] -> offsets[0..n] -------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_JPG_BLOCK) void jpeg_file_offsets_kernel(JpegArgs a) {
    __shared__ long long sh[block_scan_words<MM_JPG_BLOCK, long long>()];
    if (threadIdx.x == 0) a.offsets[0] = 0;
    (void)array_scan<true, MM_JPG_BLOCK>(a.offsets + 1, a.n, 0LL, threadIdx.x, sh);
}

// ---- write: header, stuffed bytes, EOI ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_JPG_BLOCK) void jpeg_write_kernel(JpegArgs a) {
    __shared__ int sh[4];
    const int tid = threadIdx.x, chunk = blockIdx.x, img = blockIdx.y;
    const unsigned nbits = a.frame_bits[img];
    const long long len = ((long long)nbits + 7) >> 3;
    if ((long long)chunk * MM_JPEG_CHUNK_BYTES >= len) return;                 // (the whole workgroup; a stream has a byte at least: chunk 0 stays)
    unsigned char* dst = a.files + a.offsets[img];
    if (chunk == 0) {
        const unsigned char* h = (const unsigned char*)(a.par + MM_JPG_HEADER);
        for (int i = tid; i < a.header_bytes; i += MM_JPG_BLOCK) dst[i] = h[i];
    }
    const long long byte0 = (long long)chunk * MM_JPEG_CHUNK_BYTES + tid * 4;
    const int nb = byte0 < len ? (int)min(len - byte0, 4LL) : 0;
    const unsigned w = nb ? a.raw[((size_t)img * a.chunks + chunk) * MM_JPG_CHUNK_WORDS + tid] : 0u;
    int total;
    const int before = block_prefix_excl<MM_JPG_BLOCK>(jpeg_count_ff(w, nb), tid, sh, total);
    unsigned char* p = dst + a.header_bytes + byte0 + a.chunk_ff[(size_t)img * a.chunks + chunk] + before;
    for (int i = 0; i < nb; ++i) {
        const unsigned b = (w >> (24 - 8 * i)) & 0xFFu;
        *p++ = (unsigned char)b;
        if (b == 0xFFu) *p++ = 0;
    }
    if (nb && byte0 + nb == len) { p[0] = 0xFF; p[1] = 0xD9; }
}

// ==== the round trip: frames as Image.open(file).convert('RGB' / 'L') reads them back ==========================================================
// What libjpeg's decoder makes of the file the encoder above writes, without the file: the file's content is the quantised coefficients, and
// from there the decoder is integer arithmetic (>> is arithmetic), held to Pillow with no tolerance:
//   dequantise  c[k] * table[k], table = divisor / 8: the luma table for Y and for greyscale, the chroma table for Cb and Cr
//   IDCT        jidctint's islow: CONST_BITS 13, PASS1_BITS 2, COLUMNS first with DESCALE(x, 11), then rows with DESCALE(x, 18),
//               DESCALE(x, n) = (x + (1 << (n - 1))) >> n; per pass over i0..i7
//                 even  z1 = (i2 + i6) * 4433, t2 = z1 - i6 * 15137, t3 = z1 + i2 * 6270, t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13,
//                       t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2
//                 odd   a0..a3 = i7, i5, i3, i1; z1 = a0 + a3, z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3, z5 = (z3 + z4) * 9633,
//                       a0 *= 2446, a1 *= 16819, a2 *= 25172, a3 *= 12299, z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5,
//                       z4 = z4 * -3196 + z5, a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4
//                 out   0..3 = t10 + a3, t11 + a2, t12 + a1, t13 + a0; 4..7 = t13 - a0, t12 - a1, t11 - a2, t10 - a3
//               then + 128 and clamp to 0..255.  The clamp SATURATES, as libjpeg-turbo's SIMD code does; libjpeg's C range table wraps
//               outside -384..639, which no input of the tests reaches (the host restatement counts it).
//   colour      Y is cropped to H x W.  Cb and Cr are real on hd = ceil(H / 2) rows by wd = ceil(W / 2) columns; the row above row 0 is row
//               0 and the row below row hd - 1 is row hd - 1, the last REAL downsampled row, not the padded IDCT output below it.
//               wd > 2, h2v2 fancy upsampling: input row r makes output rows 2r (neighbour: the row above) and 2r + 1 (the row below);
//                 s[x] = 3 * c[r][x] + c[neighbour][x]; out[2x] = (3 s[x] + s[x-1] + 8) >> 4; out[2x+1] = (3 s[x] + s[x+1] + 7) >> 4;
//                 at the row's ends s[-1] := s[0] and s[wd] := s[wd-1].
//               wd <= 2 (W <= 4): plain 2 x 2 replication -- libjpeg picks the plain upsampler for so narrow a component.
//               With cb and cr minus 128: R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
//               B = Y + ((116130 cb + 32768) >> 16), each clamped to 0..255.
//   greyscale   one component, 8 x 8 blocks in raster order; columns beyond W replicate the last column, rows beyond H the last row; samples
//               minus 128 through the encoder's jfdctint and quantiser (d = 8 * luma table, half away from zero), then dequantise, IDCT,
//               clamp and crop.  A block stays in registers and LDS from load to store: no greyscale file is ever formed.
// The colour path reads the int16 zigzag blocks jpeg_transform_kernel wrote, from memory -- its own pass's, or those in mm_jpeg_encode's
// workspace -- so the decoded frames cannot drift from the files.  Dummy luma blocks lie wholly outside the image and are never read.
// The arithmetic is mm_jpeg_idct.h's, shared with the file decoder; the kernels here find a lane's block or pixel, pick the divisors, skip the dummies.
//   idct      eight lanes per block: the block comes from memory into LDS, lane c dequantises column c and runs the column pass, the block
//             is transposed through LDS, lane r runs the row pass and stores row r as 8 bytes into the padded sample planes in the workspace
//             (Y 16my x 16mx, Cb and Cr 8my x 8mx per frame: 1.5 bytes per pixel).
//   pixels    one lane per dword of the (n,H,W,3) output (two pixels at most, across rows and frames alike: the output is one dense run
//             of bytes from an aligned start), or one lane per pixel of the fp32 planes: upsample, convert, store.
// No floating point but the final v / 255 of as_float, no atomics, no scratch; every output byte is a pure function of the frame.
struct JpegDecArgs {
    const short* coef; const int* par;
    unsigned char* yp; unsigned char* cp;                     // the sample planes: Y (n, 16my, 16mx); Cb and Cr (n, 2, 8my, 8mx)
    const unsigned char* grey;                                // mode L: the input (n,H,W)
    void* out;
    int n, H, W, as_float;
    int my, mx, blocks;
    int bh, bw, hd, wd;                                       // luma (grey) blocks down and across that hold pixels; real chroma rows and columns
    long long total_blocks, total_pixels;
};

template <int L>
__device__ inline JpegPlanes jpeg_frame_planes(const JpegDecArgs& a, int img) {      // the sample planes of frame img
    const JpegMcuShape m = jpeg_mcu_shape(L);
    const int mcus = a.my * a.mx;                             // (a frame's blocks are at most MM_JPEG_MAX_BLOCKS: its planes' bytes fit 32 bits)
    return {a.yp + (size_t)img * (unsigned)JpegPlanes::luma_bytes(m, mcus), a.cp + (size_t)img * (unsigned)JpegPlanes::chroma_bytes(m, mcus), a.mx, a.my};
}

// ---- idct: coefficients -> the sample planes ----------------------------------------------------------------------------------------
template <int L>
__global__ __launch_bounds__(MM_JPG_BLOCK) void jpeg_idct_kernel(JpegDecArgs a) {
    using M = JpegMcu<L>;
    __shared__ int tile[MM_JPG_BLOCK / 8][65];
    __shared__ __attribute__((aligned(16))) short zz[MM_JPG_BLOCK / 8][64];
    const int tid = threadIdx.x, lb = tid >> 3, r = tid & 7;
    const long long g = (long long)blockIdx.x * (MM_JPG_BLOCK / 8) + lb;
    const long long gc = g < a.total_blocks ? g : 0;
    const int img = (int)(gc / a.blocks), rem = (int)(gc % a.blocks);
    const int mcu = rem / M::BLOCKS, j = rem % M::BLOCKS, my = mcu / a.mx, mx = mcu % a.mx;
    const int by = M::LV * my + (j >> M::LH_SHIFT), bx = M::LH * mx + (j & (M::LH - 1));    // (luma)
    const bool live = g < a.total_blocks && !(j < M::LUMA && (by >= a.bh || bx >= a.bw));   // a dummy holds no pixel: never read
    const JpegPlanes pl = jpeg_frame_planes<L>(a, img);
    const uint2 row = jpeg_block_rows<3>(tile, zz, lb, r, live, a.coef + (size_t)g * 64, [&] { return a.par + MM_JPG_DIV + (j < M::LUMA ? 0 : 64); });
    if (!live) return;
    if (j < M::LUMA) *(uint2*)pl.luma(M::W, by * 8 + r, bx * 8) = row;
    else *(uint2*)pl.chroma(j - M::LUMA, my * 8 + r, mx * 8) = row;
}

// ---- pixels: upsample, convert, store -----------------------------------------------------------------------------------------------
// pixel p of the output, over all frames: R | G << 8 | B << 16
template <int L>
__device__ inline unsigned jpeg_pixel(const JpegDecArgs& a, long long p, int& img, int& y, int& x) {
    const int hw = a.H * a.W;
    img = (int)(p / hw);
    const int rem = (int)(p % hw);
    y = rem / a.W; x = rem % a.W;
    return jpeg_pixel_at<L>(jpeg_frame_planes<L>(a, img), a.hd, a.wd, y, x);
}

template <int L>
__global__ __launch_bounds__(MM_JPG_BLOCK) void jpeg_pixels_u8_kernel(JpegDecArgs a) {
    const long long i = (long long)blockIdx.x * MM_JPG_BLOCK + threadIdx.x, byte0 = 4 * i, bytes = 3 * a.total_pixels;
    if (byte0 >= bytes) return;
    int img, y, x;
    const unsigned w = jpeg_rgb_bytes(byte0, bytes, [&](long long p) { return jpeg_pixel<L>(a, p, img, y, x); });      // (bytes is uniform: pixel p + 1 wherever there is one)
    jpeg_store_bytes((unsigned char*)a.out, byte0, min(byte0 + 4, bytes), w);
}

template <int L>
__global__ __launch_bounds__(MM_JPG_BLOCK) void jpeg_pixels_f32_kernel(JpegDecArgs a) {
    const long long p = (long long)blockIdx.x * MM_JPG_BLOCK + threadIdx.x;
    if (p >= a.total_pixels) return;
    int img, y, x;
    const unsigned q = jpeg_pixel<L>(a, p, img, y, x);
    const size_t hw = (size_t)a.H * a.W;
    float* o = (float*)a.out + (size_t)img * 3 * hw + (size_t)y * a.W + x;
    o[0] = unquant(q & 255u); o[hw] = unquant((q >> 8) & 255u); o[2 * hw] = unquant(q >> 16);
}

// ---- grey: a mask through the encoder's transform and the decoder's, block by block ------------------------------------------------------
__global__ __launch_bounds__(MM_JPG_BLOCK) void jpeg_grey_kernel(JpegDecArgs a) {
    __shared__ int tile[MM_JPG_BLOCK / 8][65];
    const int tid = threadIdx.x, lb = tid >> 3, r = tid & 7;
    const long long g = (long long)blockIdx.x * (MM_JPG_BLOCK / 8) + lb;      // the block, over all frames, raster order in a frame
    const bool live = g < a.total_blocks;
    const long long gc = live ? g : 0;
    const int per = a.bh * a.bw, img = (int)(gc / per), rem = (int)(gc % per), by = rem / a.bw, bx = rem % a.bw;
    const size_t hw = (size_t)a.H * a.W;
    const unsigned char* f = a.grey + (size_t)img * hw + (size_t)min(by * 8 + r, a.H - 1) * a.W;
    int d[8], o[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) d[c] = (int)f[min(bx * 8 + c, a.W - 1)] - 128;
    jpeg_fdct8<true>(d, o);
#pragma unroll
    for (int c = 0; c < 8; ++c) tile[lb][r * 8 + c] = o[c];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = tile[lb][k * 8 + r];   // lane r now has column r
    jpeg_fdct8<false>(d, o);
    const int* div = a.par + MM_JPG_DIV;
#pragma unroll
    for (int k = 0; k < 8; ++k) {                             // quantise as the encoder does, dequantise as the decoder does
        const unsigned dv = (unsigned)div[k * 8 + r];
        const int m = (int)(((unsigned)abs(o[k]) + (dv >> 1)) / dv) * (int)(dv >> 3);
        d[k] = o[k] < 0 ? -m : m;
    }
    jpeg_idct8<11>(d, o);
    const uint2 row = jpeg_idct_rows(tile, lb, r, o);
    const int y = by * 8 + r, x0 = bx * 8;
    if (!live || y >= a.H) return;
    const int nx = min(8, a.W - x0);
    const unsigned w[2] = {row.x, row.y};
    const size_t at = (size_t)img * hw + (size_t)y * a.W + x0;
    if (a.as_float) {
        for (int c = 0; c < nx; ++c) ((float*)a.out)[at + c] = unquant((w[c >> 2] >> (8 * (c & 3))) & 255u);
    } else if (nx == 8 && (a.W & 3) == 0) {                  // rows of a multiple of four bytes: every block's row is two aligned words
        *(uint2*)((unsigned char*)a.out + at) = row;
    } else {
        for (int c = 0; c < nx; ++c) ((unsigned char*)a.out)[at + c] = (unsigned char)(w[c >> 2] >> (8 * (c & 3)));
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct JpegRoundtripLayout { size_t coef, yp, cp, bytes; };
__host__ JpegRoundtripLayout jpeg_roundtrip_layout(const MMJpegRoundtripDesc* d) {
    JpegRoundtripLayout l = {0, 0, 0, 256};                   // mode L needs no workspace; the query still answers 256, so that 0 stays its refusal
    if (d->mode != MM_JPEG_MODE_RGB) return l;
    const JpegMcuShape m = jpeg_mcu_shape(jpeg_layout_of(d->mode, d->sampling));
    const size_t n = (size_t)d->n, mcus = (size_t)((d->H + m.h - 1) / m.h) * ((d->W + m.w - 1) / m.w);
    Carve c;
    l.coef = c.take(d->coef ? 0 : n * mcus * m.blocks * 128);
    l.yp = c.take(n * JpegPlanes::luma_bytes(m, mcus));
    l.cp = c.take(n * JpegPlanes::chroma_bytes(m, mcus));
    l.bytes = c.at;
    return l;
}
size_t jpeg_roundtrip_workspace_bytes(const MMJpegRoundtripDesc* d) { return jpeg_roundtrip_layout(d).bytes; }
size_t jpeg_coef_at(const MMJpegModesDesc* d) { return jpeg_layout(d).coef; }

int launch_jpeg_roundtrip(const MMJpegRoundtripDesc* d, hipStream_t s) {
    const dim3 wg(MM_JPG_BLOCK);
    JpegDecArgs a = {};
    a.par = d->params; a.out = d->out;
    a.n = d->n; a.H = d->H; a.W = d->W; a.as_float = d->as_float;
    a.bh = (d->H + 7) / 8; a.bw = (d->W + 7) / 8;
    a.total_pixels = (long long)d->n * d->H * d->W;
    if (d->mode != MM_JPEG_MODE_RGB) {
        a.grey = d->frames;
        a.total_blocks = (long long)d->n * a.bh * a.bw;
        hipLaunchKernelGGL(jpeg_grey_kernel, dim3((unsigned)((a.total_blocks + MM_JPG_BLOCK / 8 - 1) / (MM_JPG_BLOCK / 8))), wg, 0, s, a);
        return launch_ok("jpeg_roundtrip");
    }
    const JpegRoundtripLayout l = jpeg_roundtrip_layout(d);
    unsigned char* ws = (unsigned char*)d->workspace;
    const int layout = jpeg_layout_of(d->mode, d->sampling);
    const JpegMcuShape m = jpeg_mcu_shape(layout);
    a.my = (d->H + m.h - 1) / m.h; a.mx = (d->W + m.w - 1) / m.w; a.blocks = a.my * a.mx * m.blocks;
    a.hd = (d->H + 1) / 2; a.wd = (d->W + 1) / 2;             // (4:2:0 reads both, 4:2:2 wd, 4:4:4 neither)
    a.total_blocks = (long long)d->n * a.blocks;
    a.yp = ws + l.yp; a.cp = ws + l.cp;
    const dim3 per_eight((unsigned)((a.total_blocks + MM_JPG_BLOCK / 8 - 1) / (MM_JPG_BLOCK / 8)));
    if (d->coef) {
        a.coef = d->coef;
    } else {                                                  // the encoder's transform, as it stands
        JpegArgs e = {};
        e.frames = d->frames; e.par = d->params; e.coef = (short*)(ws + l.coef);
        e.n = d->n; e.H = d->H; e.W = d->W;
        e.my = a.my; e.mx = a.mx; e.blocks = a.blocks;
        e.bh = a.bh; e.bw = a.bw; e.ch = a.hd;
        e.total_blocks = a.total_blocks;
        jpeg_by_layout<3>(layout, [&](auto L) { hipLaunchKernelGGL(jpeg_transform_kernel<decltype(L)::value>, per_eight, wg, 0, s, e); });
        a.coef = e.coef;
    }
    jpeg_by_layout<3>(layout, [&](auto L) {
        constexpr int V = decltype(L)::value;
        hipLaunchKernelGGL(jpeg_idct_kernel<V>, per_eight, wg, 0, s, a);
        if (d->as_float) hipLaunchKernelGGL(jpeg_pixels_f32_kernel<V>, dim3((unsigned)((a.total_pixels + MM_JPG_BLOCK - 1) / MM_JPG_BLOCK)), wg, 0, s, a);
        else hipLaunchKernelGGL(jpeg_pixels_u8_kernel<V>, dim3((unsigned)((3 * a.total_pixels + 4 * MM_JPG_BLOCK - 1) / (4 * MM_JPG_BLOCK))), wg, 0, s, a);
    });
    return launch_ok("jpeg_roundtrip");
}

int launch_jpeg(const MMJpegModesDesc* d, hipStream_t s) {
    const JpegLayout l = jpeg_layout(d);
    unsigned char* ws = (unsigned char*)d->workspace;
    JpegArgs a = {};
    a.frames = d->frames; a.par = d->params;
    a.offsets = (long long*)(ws + l.offsets); a.files = ws + l.files; a.coef = (short*)(ws + l.coef); a.bits = (unsigned*)(ws + l.bits);
    a.frame_bits = (unsigned*)(ws + l.frame_bits); a.raw = (unsigned*)(ws + l.raw); a.chunk_ff = (unsigned*)(ws + l.chunk_ff);
    a.n = d->n; a.H = d->H; a.W = d->W; a.header_bytes = d->header_bytes;
    a.my = l.my; a.mx = l.mx; a.blocks = l.blocks; a.chunks = l.chunks;
    a.bh = (d->H + 7) / 8; a.bw = (d->W + 7) / 8; a.ch = (d->H + 1) / 2;
    a.total_blocks = (long long)d->n * l.blocks;
    if (hipMemsetAsync(a.raw, 0, (size_t)d->n * l.chunks * MM_JPEG_CHUNK_BYTES, s) != hipSuccess) return launch_ok("jpeg_zero");
    const dim3 wg(MM_JPG_BLOCK), per_frame((unsigned)d->n), per_chunk((unsigned)l.chunks, (unsigned)d->n);
    const unsigned per_block = (unsigned)((a.total_blocks + MM_JPG_BLOCK - 1) / MM_JPG_BLOCK);
    jpeg_by_layout(l.layout, [&](auto L) {
        constexpr int V = decltype(L)::value;
        hipLaunchKernelGGL(jpeg_transform_kernel<V>, dim3((unsigned)((a.total_blocks + MM_JPG_BLOCK / 8 - 1) / (MM_JPG_BLOCK / 8))), wg, 0, s, a);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(jpeg_code_kernel<V, false>), dim3(per_block), wg, 0, s, a);
        hipLaunchKernelGGL(jpeg_bit_offsets_kernel, per_frame, wg, 0, s, a);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(jpeg_code_kernel<V, true>), dim3(per_block), wg, 0, s, a);
    });
    hipLaunchKernelGGL(jpeg_count_ff_kernel, per_chunk, wg, 0, s, a);
    hipLaunchKernelGGL(jpeg_place_kernel, per_frame, wg, 0, s, a);
    hipLaunchKernelGGL(jpeg_file_offsets_kernel, dim3(1), wg, 0, s, a);
    hipLaunchKernelGGL(jpeg_write_kernel, per_chunk, wg, 0, s, a);
    return launch_ok("jpeg");
}

}  // namespace mm
