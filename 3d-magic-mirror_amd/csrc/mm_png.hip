// mm_png.hip -- 8-bit device frames (n,H,W,C), C = 1 / 3 / 4 (grey, RGB, RGBA), as n PNG files, for gfx950: what the reference does on the host per
// image with vutils.save_image(..., '.png') and Image.save(..., 'PNG') (trainer.py:564-607,793,933, the *_single_img.py, show_camera.py and
// show_rainbow2.py outputs).  PNG is lossless: a decoder returns the frames to the bit.  The file is this project's own, fully specified
// (no other writer's bytes are a target), and every decoder reads it.  Integer arithmetic only; every atomic is an integer OR or XOR, so
// their order cannot matter and every byte is a pure function of the frames (bitwise reproducible).  Per frame, in order:
//   file       89 50 4E 47 0D 0A 1A 0A; IHDR (W, H u32be, depth 8, colour type 0 / 2 / 6, 0, 0, 0); ONE IDAT; IEND.  A chunk is its data's
//              length u32be, its type, its data, CRC-32 of type + data u32be.
//   filter     the stream S is H rows of 1 + W*C bytes: the filter type, then the filtered row.  With bpp = C, a is the byte bpp to the
//              left, b the byte above, c above-left, 0 outside the image, all of the RAW rows.  Types 0 None, 1 Sub x - a, 2 Up x - b,
//              3 Average x - (a + b) / 2, 4 Paeth (p = a + b - c; a if |p-a| <= |p-b| and |p-a| <= |p-c|, else b if |p-b| <= |p-c|, else c),
//              all mod 256.  Adaptive: per row the type with the smallest sum of (v < 128 ? v : 256 - v) over the filtered bytes, ties to
//              the lowest type; or one forced type for every row.
//   zlib       78 01, the deflate blocks, zero bits up to a byte, Adler-32 of S u32be.
//   deflate    S is cut into segments of `segment` bytes (the last may be shorter), each ONE block with the fixed Huffman codes: BFINAL
//              (1 on the last only), 1, 0, the symbols, end-of-block (256).  Blocks follow each other bit by bit.
//   matching   inside a segment [s, e), greedy, never reaching before s.  At i with i + 3 <= e: j is the LATEST position in [s, i) with
//              S[j..j+3) == S[i..i+3); L the longest length <= min(258, e - i) with S[j+k] == S[i+k] for k < L (overlap allowed).  With
//              such a j the match (L, i - j) is emitted and i += L; otherwise the literal S[i] and i += 1.
//   codes      RFC 1951 3.2.6: symbols 0-143 are 8 bits 0x30 + v, 144-255 9 bits 0x190 + (v - 144), 256-279 7 bits v - 256, 280-287 8 bits
//              0xC0 + (v - 280); a distance code is 5 bits.  Huffman codes enter the LSB-first stream most significant bit first, extra bits
//              least significant bit first.  Lengths 3..10 are codes 257..264 without extra bits, 258 is code 285 without; between them a
//              code has e = floor(log2(L - 3)) - 2 extra bits, four codes to every e.  Distances 1..4 are codes 0..3; beyond them a code
//              has e = floor(log2(D - 1)) - 1 extra bits, two codes to every e.
//
// Seven launches and one memset on the caller's stream, nothing synchronises.  What bounds each pass:
//   filter     a workgroup per row.  Every lane reads x, a, b and c of its bytes (this row and the one above, so a frame's byte comes in a
//              handful of times, from the caches after the first), forms the five costs, the waves fold them (DPP) and the workgroup adds the
//              four waves'; a second walk writes the chosen type's bytes once.  Bound by the byte loads: memory traffic is 2 bytes per byte.
//   code       a wave per segment, its bytes and its table (trigram -> latest position, open addressing over 16-bit positions, a power of two
//              of at least 2 * segment slots; a hit is confirmed against the bytes themselves, so the table is exact) in LDS: 6 bytes a byte
//              of the segment, 40 KiB at MM_PNG_MAX_SEGMENT, so 4 to 32 waves share a CU's 160 KiB.  While the lanes load the bytes they form
//              the segment's Adler sums, sum d and sum (len - i) d, each mod 65521.  The walk is serial by nature: an LDS probe per byte, for
//              the bytes inside a match too (they are later positions' predecessors).  All 64 lanes walk in step, so nothing diverges (a lane
//              per segment was measured first: the lanes' walks serialise, and the call took 28.6 ms where it now takes 12.9), and a match's length is found 64 bytes
//              at a time (ballot).  Bound by LDS latency; the waves in flight hide it.  The symbols leave as the segment's own bit stream in
//              its slot of the workspace, sized for the exact worst case (3 + 9 len + 7 bits: a match never costs more than its bytes would
//              as literals), with the bit count.
//   offsets    a workgroup per frame scans the segments' bit counts (array_scan of mm_stream.h) and combines the Adler sums:
//              s1 = 1 + sum_k sum_k, s2 = |S| + sum_k (w_k + sum_k * bytes after segment k), mod 65521 in 64 bits.
//   pack       a lane per 32-bit word of a segment's stream ORs it into the frame's zeroed stream at the bit offset.
//   place      one workgroup scans the frames' lengths into the n + 1 offsets at the head of the workspace.
//   write      the framing and the IDAT's bytes; a lane takes the raw CRC of its piece of MM_PNG_CRC_PIECE bytes of type + data (the first
//              piece starts from 0xFFFFFFFF) and multiplies it by x^(8 * bytes after the piece) mod P (carry-less, by squaring: CRC is
//              linear over GF(2)); the waves' XORs meet in one word per frame.
//   seal       that word, inverted, behind the IDAT's data.
// (PngBits is GifBits of mm_gif.hip: LSB first, a private slot, plain stores.  It stays here so that this file only adds.)
#include <hip/hip_runtime.h>

#include "mm_device.h"
#include "mm_stream.h"                                        // array_scan, Carve: what the encoders share

#define MM_PNG_BLOCK 256
#define MM_PNG_EMPTY 0xFFFFu
#define MM_PNG_POLY 0xEDB88320u
#define MM_PNG_HEAD 41                                        // signature 8, IHDR 25, the IDAT's length and type 8: where its data starts

namespace mm {

struct PngLayout {
    long long row, stream, segs, all_segs;                    // bytes of a filtered row and of a frame's S; segments of a frame, of the call
    int slot_words, table_slots, table_shift;                 // a segment's stream; its table (slots, 32 - log2)
    long long raw_words, deflate_cap;                         // a frame's packed stream in words; the most bytes its deflate blocks take
    size_t file_cap;
    size_t offsets, files, raw, crc, frame, seg_bits, seg_sums, S, slots, zero_bytes, bytes;      // byte offsets into the workspace
};
__host__ PngLayout png_layout(const MMPngDesc* d) {
    PngLayout l;
    const size_t n = (size_t)d->n;
    l.row = 1 + (long long)d->W * d->channels;
    l.stream = l.row * d->H;
    l.segs = (l.stream + d->segment - 1) / d->segment;
    l.all_segs = l.segs * d->n;
    l.slot_words = (10 + 9 * d->segment + 31) / 32;
    l.table_slots = 2;
    while (l.table_slots < 2 * d->segment) l.table_slots *= 2;
    l.table_shift = 32;
    for (int s = l.table_slots; s > 1; s >>= 1) --l.table_shift;
    const long long frame_bits = 10 * l.segs + 9 * l.stream;
    l.raw_words = (frame_bits + 31) / 32 + 1;
    l.deflate_cap = (frame_bits + 7) / 8;
    l.file_cap = (size_t)(8 + 25 + 12 + (2 + l.deflate_cap + 4) + 12);
    Carve c;
    l.offsets = c.take((n + 1) * 8);                          // where each file starts, and the end of the last: what a caller copies first
    l.files = c.take(n * l.file_cap);
    l.raw = c.take(n * (size_t)l.raw_words * 4);
    l.crc = c.take(n * 4);
    l.zero_bytes = c.at - l.raw;                              // the streams and the CRC words start as zeros
    l.frame = c.take(n * 16);                                 // per frame: its deflate bits, its Adler-32
    l.seg_bits = c.take(n * (size_t)l.segs * 8);
    l.seg_sums = c.take(n * (size_t)l.segs * 8);
    l.S = c.take(n * (size_t)l.stream);
    l.slots = c.take(n * (size_t)l.segs * l.slot_words * 4);
    l.bytes = c.at;
    return l;
}
size_t png_workspace_bytes(const MMPngDesc* d) { return png_layout(d).bytes; }
size_t png_files_at(const MMPngDesc* d) { return png_layout(d).files; }
// the most bytes one frame's IDAT holds, and the segments of the whole call: what mm_abi.hip refuses beyond 2^31 - 1
long long png_idat_cap(const MMPngDesc* d) { return 2 + png_layout(d).deflate_cap + 4; }
long long png_all_segs(const MMPngDesc* d) { return png_layout(d).all_segs; }

struct PngFrame { unsigned long long bits; unsigned adler, pad; };

struct PngArgs {
    const unsigned char* frames;
    long long* offsets; unsigned char* files; unsigned* raw; unsigned* crc; PngFrame* frame;
    unsigned long long* seg_bits; unsigned long long* seg_sums; unsigned char* S; unsigned* slots;
    int n, H, W, C, filter, segment;
    long long row, stream, segs, all_segs, raw_words;
    int slot_words, table_slots, table_shift;
    unsigned x2n[32];                                         // x^(2^k) mod P, reflected as the CRC register is
};

// ---- filter: a workgroup per row ------------------------------------------------------------------------------------------------------------
struct PngNear { int x, a, b, c; };
__device__ inline PngNear png_near(const unsigned char* cur, const unsigned char* prev, int t, int bpp) {
    PngNear p;
    p.x = cur[t];
    p.a = t >= bpp ? cur[t - bpp] : 0;
    p.b = prev ? prev[t] : 0;
    p.c = prev && t >= bpp ? prev[t - bpp] : 0;
    return p;
}
__device__ inline int png_paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}
__device__ inline int png_filtered(const PngNear& p, int type) {
    const int pred = type == 0 ? 0 : type == 1 ? p.a : type == 2 ? p.b : type == 3 ? (p.a + p.b) >> 1 : png_paeth(p.a, p.b, p.c);
    return (p.x - pred) & 255;
}

__global__ __launch_bounds__(MM_PNG_BLOCK) void png_filter_kernel(PngArgs a) {
    __shared__ unsigned red[MM_PNG_BLOCK / 64][5];
    const int tid = threadIdx.x, y = blockIdx.x, frame = blockIdx.y;
    const int rb = a.W * a.C;
    const unsigned char* cur = a.frames + ((size_t)frame * a.H + y) * rb;
    const unsigned char* prev = y > 0 ? cur - rb : nullptr;
    unsigned char* out = a.S + (size_t)frame * a.stream + (size_t)y * a.row;
    int type = a.filter;
    if (type < 0) {                                           // (uniform: the call's)
        unsigned cost[5] = {0, 0, 0, 0, 0};
        for (int t = tid; t < rb; t += MM_PNG_BLOCK) {
            const PngNear p = png_near(cur, prev, t, a.C);
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int v = png_filtered(p, k);
                cost[k] += (unsigned)(v < 128 ? v : 256 - v);
            }
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const unsigned w = wave_reduce(cost[k], [](unsigned p, unsigned q) { return p + q; });
            if ((tid & 63) == 0) red[tid >> 6][k] = w;
        }
        __syncthreads();
        unsigned best = 0xFFFFFFFFu;
        type = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const unsigned c = red[0][k] + red[1][k] + red[2][k] + red[3][k];
            if (c < best) { best = c; type = k; }             // (a tie keeps the lower type)
        }
    }
    if (tid == 0) out[0] = (unsigned char)type;
    for (int t = tid; t < rb; t += MM_PNG_BLOCK) out[1 + t] = (unsigned char)png_filtered(png_near(cur, prev, t, a.C), type);
}

// ---- code: a wave per segment ---------------------------------------------------------------------------------------------------------------
// Every lane of the wave walks the segment in step (the same reads, broadcast by the LDS; the same registers), so the walk diverges nowhere
// and the lanes are at hand where it forks out: a match's length is found 64 bytes at a time.  Lane 0 alone stores.
struct PngBits {
    unsigned long long acc = 0;
    int nacc = 0;
    unsigned* out;
    unsigned words = 0;
    bool stores;                                              // lane 0
    __device__ inline void put(unsigned code, int width) {    // width <= 16
        acc |= (unsigned long long)code << nacc;
        nacc += width;
        if (nacc >= 32) { if (stores) out[words] = (unsigned)acc; ++words; acc >>= 32; nacc -= 32; }
    }
    __device__ inline void huff(unsigned code, int width) { put(__brev(code) >> (32 - width), width); }      // most significant bit first
    __device__ inline void symbol(unsigned v) {               // a literal / length symbol 0..287
        if (v < 144) huff(0x30 + v, 8);
        else if (v < 256) huff(0x190 + (v - 144), 9);
        else if (v < 280) huff(v - 256, 7);
        else huff(0xC0 + (v - 280), 8);
    }
    __device__ inline void match(int L, int D) {
        if (L <= 10) symbol(254 + L);
        else if (L == 258) symbol(285);
        else {
            const int m = L - 3, e = 29 - __clz(m);           // floor(log2 m) - 2
            symbol(257 + 4 * e + 4 + ((m >> e) & 3));
            put((unsigned)m & ((1u << e) - 1u), e);
        }
        if (D <= 4) huff(D - 1, 5);
        else {
            const int m = D - 1, e = 30 - __clz(m);           // floor(log2 m) - 1
            huff(2 * e + 2 + ((m >> e) & 1), 5);
            put((unsigned)m & ((1u << e) - 1u), e);
        }
    }
    __device__ inline unsigned long long finish() {
        const unsigned long long bits = (unsigned long long)words * 32 + nacc;
        if (nacc > 0 && stores) out[words] = (unsigned)acc;
        return bits;
    }
};

// position i enters the table; what stood there for its trigram before (the latest earlier position with these three bytes), or MM_PNG_EMPTY
__device__ inline unsigned png_enter(unsigned short* table, const unsigned char* px, int i, int shift, unsigned mask, bool stores) {
    const unsigned tri = px[i] | px[i + 1] << 8 | px[i + 2] << 16;
    unsigned h = (tri * 2654435761u) >> shift;
    unsigned e;
    while ((e = table[h]) != MM_PNG_EMPTY && (px[e] | px[e + 1] << 8 | px[e + 2] << 16) != tri) h = (h + 1) & mask;
    if (stores) table[h] = (unsigned short)i;
    return e;
}

__global__ __launch_bounds__(64) void png_code_kernel(PngArgs a) {
    extern __shared__ unsigned png_lds[];
    const int lane = threadIdx.x;
    const bool stores = lane == 0;
    unsigned short* table = (unsigned short*)png_lds;
    unsigned char* px = (unsigned char*)(table + a.table_slots);
    const long long seg = blockIdx.x, frame = seg / a.segs, s = seg - frame * a.segs;
    const int len = (int)min((long long)a.segment, a.stream - s * a.segment);
    const unsigned char* src = a.S + (size_t)frame * a.stream + (size_t)s * a.segment;
    for (int i = lane; i < a.table_slots; i += 64) table[i] = MM_PNG_EMPTY;
    unsigned sum = 0, w = 0;                                  // the segment's Adler sums; a lane's: at most 128 bytes, 128 * 8192 * 255 < 2^32
    for (int i = lane; i < len; i += 64) { const unsigned d = src[i]; px[i] = (unsigned char)d; sum += d; w += (unsigned)(len - i) * d; }
    w %= 65521u;
    sum = wave_reduce(sum, [](unsigned p, unsigned q) { return p + q; });
    w = wave_reduce(w, [](unsigned p, unsigned q) { return p + q; });
    if (stores) a.seg_sums[seg] = (unsigned long long)(sum % 65521u) | (unsigned long long)(w % 65521u) << 32;
    __syncthreads();
    const unsigned mask = (unsigned)a.table_slots - 1u;
    PngBits bits;
    bits.out = a.slots + (size_t)seg * a.slot_words;
    bits.stores = stores;
    bits.put((s == a.segs - 1 ? 1u : 0u) | 2u, 3);           // BFINAL, then BTYPE 01 least significant bit first
    int i = 0;
    while (i < len) {
        const unsigned j = i + 3 <= len ? png_enter(table, px, i, a.table_shift, mask, stores) : MM_PNG_EMPTY;
        if (j == MM_PNG_EMPTY) { bits.symbol(px[i]); ++i; continue; }
        const int most = min(258, len - i);
        int L = 3;
        while (L < most) {                                    // 64 bytes a step
            const int k = L + lane;
            const unsigned long long eq = __ballot(k < most && px[j + k] == px[i + k]);
            const int run = eq == ~0ull ? 64 : __ffsll((long long)~eq) - 1;
            L += run;
            if (run < 64) break;
        }
        bits.match(L, i - (int)j);
        const int end = i + L;
        for (++i; i < end; ++i)
            if (i + 3 <= len) (void)png_enter(table, px, i, a.table_shift, mask, stores);
    }
    bits.symbol(256);
    const unsigned long long nbits = bits.finish();
    if (stores) a.seg_bits[seg] = nbits;
}

// ---- offsets: per frame, the segments' bit counts -> bit offsets, in place; the frame's bits, Adler-32 and length in the file ---------------
__global__ __launch_bounds__(MM_PNG_BLOCK) void png_bit_offsets_kernel(PngArgs a) {
    __shared__ unsigned long long sh[block_scan_words<MM_PNG_BLOCK, unsigned long long>()];
    const int tid = threadIdx.x, frame = blockIdx.x;
    const unsigned long long carry = array_scan<false, MM_PNG_BLOCK>(a.seg_bits + (size_t)frame * a.segs, a.segs, 0ull, tid, sh);
    unsigned long long s1 = 0, s2 = 0;
    for (long long k = tid; k < a.segs; k += MM_PNG_BLOCK) {
        const unsigned long long v = a.seg_sums[(size_t)frame * a.segs + k];
        const unsigned long long sum = v & 0xFFFFFFFFull, w = v >> 32;
        const long long after = a.stream - min((k + 1) * a.segment, a.stream);
        s1 = (s1 + sum) % 65521ull;
        s2 = (s2 + w + sum * (unsigned long long)(after % 65521)) % 65521ull;
    }
    __syncthreads();                                          // (the scan's last pass may still be read)
    sh[tid] = s1 | s2 << 32;
    __syncthreads();
    if (tid == 0) {
        s1 = 1; s2 = (unsigned long long)(a.stream % 65521);
        for (int t = 0; t < MM_PNG_BLOCK; ++t) { s1 += sh[t] & 0xFFFFFFFFull; s2 += sh[t] >> 32; }
        PngFrame f;
        f.bits = carry; f.adler = (unsigned)(s2 % 65521ull) << 16 | (unsigned)(s1 % 65521ull); f.pad = 0;
        a.frame[frame] = f;
        a.offsets[frame + 1] = 8 + 25 + 12 + (2 + (long long)((carry + 7) >> 3) + 4) + 12;
    }
}

// ---- pack: a segment's words into its frame's stream ------------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_PNG_BLOCK) void png_pack_kernel(PngArgs a) {
    const long long seg = blockIdx.x;
    const long long frame = seg / a.segs, s = seg - frame * a.segs;
    const unsigned long long off = a.seg_bits[seg];
    const unsigned long long nbits = (s + 1 < a.segs ? a.seg_bits[seg + 1] : a.frame[frame].bits) - off;
    const int w = blockIdx.y * MM_PNG_BLOCK + threadIdx.x;
    if (w >= a.slot_words || (unsigned long long)w * 32 >= nbits) return;
    const unsigned v = a.slots[(size_t)seg * a.slot_words + w];
    if (!v) return;
    const unsigned long long at = off + (unsigned long long)w * 32;
    unsigned* dst = a.raw + (size_t)frame * a.raw_words + (at >> 5);
    const int sh = (int)(at & 31);
    atomicOr(dst, v << sh);
    if (sh && (v >> (32 - sh))) atomicOr(dst + 1, v >> (32 - sh));
}

// ---- place: the frames' lengths in offsets[1..n] -> where each starts and the last ends, offsets[0..n] -------------------------------------
__global__ __launch_bounds__(MM_PNG_BLOCK) void png_place_kernel(PngArgs a) {
    __shared__ long long sh[block_scan_words<MM_PNG_BLOCK, long long>()];
    const int tid = threadIdx.x;
    if (tid == 0) a.offsets[0] = 0;
    (void)array_scan<true, MM_PNG_BLOCK>(a.offsets + 1, a.n, 0ll, tid, sh);
}

// ---- write: the framing, the IDAT's bytes and its CRC-32 ----------------------------------------------------------------------------------
// a * b mod P, both reflected (bit 31 is x^0), as the CRC register is
__host__ __device__ inline unsigned png_mulmod(unsigned a, unsigned b) {
    unsigned p = 0;
    for (int k = 31; k >= 0; --k) {
        if ((a >> k) & 1u) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? MM_PNG_POLY : 0u);
    }
    return p;
}
// x^(8 * bytes) mod P
__device__ inline unsigned png_xpow(const unsigned* x2n, unsigned long long bytes) {
    unsigned p = 0x80000000u;
    for (int k = 3; bytes; bytes >>= 1, ++k)
        if (bytes & 1ull) p = png_mulmod(x2n[k & 31], p);
    return p;
}
__device__ inline unsigned png_crc_bytes(const unsigned* table, unsigned crc, const unsigned char* p, int count) {
    for (int i = 0; i < count; ++i) crc = table[(crc ^ p[i]) & 255u] ^ (crc >> 8);
    return crc;
}
__device__ inline void png_u32be(unsigned char* p, unsigned v) { p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v; }

// byte k of what the IDAT's CRC covers: "IDAT", 78 01, the deflate bytes, the Adler-32
__device__ inline unsigned png_idat_byte(long long k, const unsigned char* raw, long long deflate, unsigned adler) {
    if (k < 4) return k == 0 ? 'I' : k == 1 ? 'D' : k == 2 ? 'A' : 'T';
    if (k < 6) return k == 4 ? 0x78u : 0x01u;
    if (k < 6 + deflate) return raw[k - 6];
    return (adler >> (8 * (3 - (int)(k - 6 - deflate)))) & 255u;
}

__global__ __launch_bounds__(MM_PNG_BLOCK) void png_write_kernel(PngArgs a) {
    __shared__ unsigned table[256];
    const int tid = threadIdx.x, frame = blockIdx.y;
    {
        unsigned c = (unsigned)tid;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? MM_PNG_POLY : 0u);
        table[tid] = c;
    }
    __syncthreads();
    const PngFrame f = a.frame[frame];
    const long long deflate = (long long)((f.bits + 7) >> 3), covered = 4 + 2 + deflate + 4;      // type + data
    unsigned char* dst = a.files + a.offsets[frame];
    const unsigned char* raw = (const unsigned char*)(a.raw + (size_t)frame * a.raw_words);
    if (blockIdx.x == 0 && tid == 0) {
        const unsigned char head[29] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A, 0, 0, 0, 13, 'I', 'H', 'D', 'R',
                                        (unsigned char)(a.W >> 24), (unsigned char)(a.W >> 16), (unsigned char)(a.W >> 8), (unsigned char)a.W,
                                        (unsigned char)(a.H >> 24), (unsigned char)(a.H >> 16), (unsigned char)(a.H >> 8), (unsigned char)a.H,
                                        8, (unsigned char)(a.C == 1 ? 0 : a.C == 3 ? 2 : 6), 0, 0, 0};
        for (int i = 0; i < 29; ++i) dst[i] = head[i];
        png_u32be(dst + 29, ~png_crc_bytes(table, 0xFFFFFFFFu, head + 12, 17));
        png_u32be(dst + 33, (unsigned)(covered - 4));
        const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        for (int i = 0; i < 12; ++i) dst[37 + covered + 4 + i] = iend[i];
    }
    constexpr long long SPAN = (long long)MM_PNG_BLOCK * MM_PNG_CRC_PIECE;
    for (long long base = (long long)blockIdx.x * SPAN; base < covered; base += (long long)gridDim.x * SPAN) {
        const long long stop = min(base + SPAN, covered);
        for (long long k = base + tid; k < stop; k += MM_PNG_BLOCK) dst[37 + k] = (unsigned char)png_idat_byte(k, raw, deflate, f.adler);
        const long long p0 = base + (long long)tid * MM_PNG_CRC_PIECE, p1 = min(p0 + MM_PNG_CRC_PIECE, covered);
        unsigned crc = 0;
        if (p0 < covered) {
            crc = p0 == 0 ? 0xFFFFFFFFu : 0u;
            for (long long k = p0; k < p1; ++k) crc = table[(crc ^ png_idat_byte(k, raw, deflate, f.adler)) & 255u] ^ (crc >> 8);
            crc = png_mulmod(png_xpow(a.x2n, (unsigned long long)(covered - p1)), crc);
        }
        crc = wave_reduce(crc, [](unsigned p, unsigned q) { return p ^ q; });
        if ((tid & 63) == 0 && crc) atomicXor(a.crc + frame, crc);
    }
}

// ---- seal: the IDAT's CRC ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_PNG_BLOCK) void png_seal_kernel(PngArgs a) {
    const int frame = blockIdx.x * MM_PNG_BLOCK + threadIdx.x;
    if (frame >= a.n) return;
    const long long deflate = (long long)((a.frame[frame].bits + 7) >> 3);
    png_u32be(a.files + a.offsets[frame] + MM_PNG_HEAD + 2 + deflate + 4, ~a.crc[frame]);
}

int launch_png(const MMPngDesc* d, hipStream_t s) {
    const PngLayout l = png_layout(d);
    PngArgs a = {};
    unsigned char* ws = (unsigned char*)d->workspace;
    a.frames = d->frames;
    a.offsets = (long long*)(ws + l.offsets); a.files = ws + l.files; a.raw = (unsigned*)(ws + l.raw); a.crc = (unsigned*)(ws + l.crc);
    a.frame = (PngFrame*)(ws + l.frame); a.seg_bits = (unsigned long long*)(ws + l.seg_bits); a.seg_sums = (unsigned long long*)(ws + l.seg_sums);
    a.S = ws + l.S; a.slots = (unsigned*)(ws + l.slots);
    a.n = d->n; a.H = d->H; a.W = d->W; a.C = d->channels; a.filter = d->filter; a.segment = d->segment;
    a.row = l.row; a.stream = l.stream; a.segs = l.segs; a.all_segs = l.all_segs; a.raw_words = l.raw_words;
    a.slot_words = l.slot_words; a.table_slots = l.table_slots; a.table_shift = l.table_shift;
    unsigned p = 1u << 30;                                    // x^1
    a.x2n[0] = p;
    for (int k = 1; k < 32; ++k) a.x2n[k] = p = png_mulmod(p, p);
    const dim3 wg(MM_PNG_BLOCK);
    if (hipMemsetAsync(a.raw, 0, l.zero_bytes, s) != hipSuccess) return launch_ok("png_zero");
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)d->H, (unsigned)d->n), wg, 0, s, a);
    const size_t lds = (size_t)l.table_slots * 2 + ((d->segment + 3) & ~3);        // at most 40 KiB
    hipLaunchKernelGGL(png_code_kernel, dim3((unsigned)l.all_segs), dim3(64), lds, s, a);
    hipLaunchKernelGGL(png_bit_offsets_kernel, dim3((unsigned)d->n), wg, 0, s, a);
    hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)l.all_segs, (unsigned)((l.slot_words + MM_PNG_BLOCK - 1) / MM_PNG_BLOCK)), wg, 0, s, a);
    hipLaunchKernelGGL(png_place_kernel, dim3(1), wg, 0, s, a);
    const long long spans = (6 + l.deflate_cap + 4 + (long long)MM_PNG_BLOCK * MM_PNG_CRC_PIECE - 1) / ((long long)MM_PNG_BLOCK * MM_PNG_CRC_PIECE);
    hipLaunchKernelGGL(png_write_kernel, dim3((unsigned)min(spans, 256LL), (unsigned)d->n), wg, 0, s, a);
    hipLaunchKernelGGL(png_seal_kernel, dim3((unsigned)((d->n + MM_PNG_BLOCK - 1) / MM_PNG_BLOCK)), wg, 0, s, a);
    return launch_ok("png");
}

}  // namespace mm
