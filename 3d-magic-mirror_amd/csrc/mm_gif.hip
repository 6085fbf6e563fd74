// mm_gif.hip -- 8-bit device frames (n,H,W,3) as ONE animated GIF89a file, for gfx950: what the reference's render loops do on the host per
// frame with imageio.get_writer(path, mode='I') ... writer.append_data((image * 255).astype(np.uint8)) (trainer.py:616-695,
// show_rainbow2.py:377-470, show_camera.py:396-500, *_single_img.py:372-390).  The file is this project's own, fully specified (no other
// writer's bytes are a target), and every decoder reads it.  Integer arithmetic only; every atomic is an integer add, min, max or OR, so
// their order cannot matter and every byte is a pure function of the frames (bitwise reproducible).  In order:
//   histogram  over all frames of the call: bin = (r>>3)<<10 | (g>>3)<<5 | (b>>3), 32768 bins, each a pixel count and the sums of r&7, g&7
//              and b&7 (n*H*W < 2^29, so 7 * count stays inside 32 bits).
//   palette    median cut over the non-empty bins.  Box 0 holds them all.  While there are fewer than 256 boxes and some box has two
//              non-empty bins or more: split the one with the largest pixel count among those (ties: the lowest box index) along the axis
//              with the largest max - min bin coordinate over its non-empty bins (ties: g, then r, then b) at k, the smallest coordinate in
//              [min, max-1] whose cumulative marginal count from min reaches (count+1)/2 (max-1 if none does); bins with coordinate <= k
//              keep the box, the others get index = boxes so far.  Entry i, per channel: (2 s + c) / (2 c) with c = sum count and
//              s = sum (count * (coord << 3) + low_sum) over the box's bins, 64 bits; unused entries are 0,0,0.
//   indices    a pixel's index is the box of its bin: the per-bin box array is the lookup table, there is no nearest-colour search.
//   LZW        a frame's indices in raster order are cut into segments of `segment` pixels (the last may be shorter) that code
//              independently.  The frame's stream opens with Clear (256) at 9 bits.  A segment codes greedily, longest match, with a fresh
//              dictionary: next = 258, width = 9; when a new entry receives code next: if next == 1 << width and width < 12 the width grows
//              by one, then next += 1.  After the segment's last data code the same test is applied once more (the decoder adds one more
//              entry there); then Clear at that width, or EOI (257) after the frame's last segment.  Codes are packed LSB first, the frame's
//              last byte is zero-padded.  segment <= 3838: the dictionary can never fill.
//   file       "GIF89a", W, H, 0xF7, 0, 0, the 768 palette bytes, with a loop count 21 FF 0B "NETSCAPE2.0" 03 01 <loop u16le> 00; per frame
//              21 F9 04 04 <delay u16le> 00 00, 2C 0 0 0 0 <W> <H> 00, 08, the stream in sub-blocks of up to 255 bytes each behind its
//              length byte (stream byte j sits at j + j / 255 + 1), 00; finally 3B.
//
// Eight launches and one memset on the caller's stream, nothing synchronises:
//   histogram  a lane walks 64 consecutive pixels and hands its run on at a change of bin; the runs still open at the end are summed over
//              the wave for the bin of its first lane (a render sheet's white).  Runs meet in a table of 2048 bins in the workgroup's LDS
//              (a run that finds no slot in eight probes goes to memory directly); the table's bins leave as two 64-bit atomics each.
//   median cut ONE workgroup of 1024.  The non-empty bins are compacted through LDS and then live in registers, 32 entries to a lane (bin,
//              box, pixel count); the boxes' count, bin count and extents live in LDS.  A split is an argmax over the boxes, a marginal
//              pass and a reassign pass over the lane's entries; a lane gathers its entries' statistics, a wave its lanes', before one lane touches the shared ones.
//   index      a lane per pixel through the 32 KiB table.
//   code       a lane per segment, its pixels and its open-addressed dictionary (prefix << 8 | byte -> code, a power of two of at least
//              2 * segment 32-bit slots) in LDS, as many segments to a workgroup of one wave as fit 64 KiB.  The chain is serial by nature:
//              an LDS probe per pixel.  The codes leave as the segment's own bit stream in its slot of the workspace, sized for the exact
//              worst case (every code new), with the bit count.
//   offsets    a workgroup per frame scans the segments' bit counts (array_scan of mm_stream.h, as place does and the JPEG encoder's scans).
//   pack       a lane per 32-bit word of a segment's stream ORs it into the frame's zeroed stream at the bit offset.
//   place      one workgroup scans the frames' lengths; the file's length goes to byte 0 of the workspace.
//   write      the file's head, the frames' heads, the sub-blocks with their length bytes, terminators and the trailer.
#include <hip/hip_runtime.h>

#include "mm_device.h"
#include "mm_stream.h"                                        // array_scan, Carve: what the encoders share

#define MM_GIF_BLOCK 256
#define MM_GIF_CUT_BLOCK 1024
#define MM_GIF_BINS 32768
#define MM_GIF_RUN 64                                         // pixels a lane of the histogram walks
#define MM_GIF_CODE_LDS (64 * 1024)
#define MM_GIF_HIST_LOG2 11                                   // the histogram's table per workgroup: 2048 bins, 40 KiB
#define MM_GIF_HIST_SLOTS (1 << MM_GIF_HIST_LOG2)

namespace mm {

// bits a segment of len pixels codes to at most: len + 1 codes, all data codes new, code k at 9 + (k >= 255) + (k >= 767) + (k >= 1791) bits
__host__ inline long long gif_worst_bits(long long len) {
    const long long codes = len + 1;
    long long bits = 9 * codes;
    if (codes > 255) bits += codes - 255;
    if (codes > 767) bits += codes - 767;
    if (codes > 1791) bits += codes - 1791;
    return bits;
}

struct GifLayout {
    long long pixels, segs;                                   // of one frame
    int slot_words, table_slots, table_shift, group;          // a segment's stream; its dictionary (slots, 32 - log2); segments per workgroup
    long long raw_words;                                      // a frame's packed stream
    int head;                                                 // bytes in front of the first frame
    size_t file_cap;
    size_t total, file, hist, lut, raw, seg_bits, frame_len, slots, zero_bytes, bytes;      // byte offsets into the workspace
};
__host__ GifLayout gif_layout(const MMGifDesc* d) {
    GifLayout l;
    const size_t n = (size_t)d->n;
    l.pixels = (long long)d->H * d->W;
    l.segs = (l.pixels + d->segment - 1) / d->segment;
    l.slot_words = (int)((gif_worst_bits(d->segment) + 9 + 31) / 32) + 1;
    l.table_slots = 2;
    while (l.table_slots < 2 * d->segment) l.table_slots *= 2;
    l.table_shift = 32;
    for (int s = l.table_slots; s > 1; s >>= 1) --l.table_shift;
    l.group = MM_GIF_CODE_LDS / (l.table_slots * 4 + ((d->segment + 3) & ~3));
    if (l.group > 64) l.group = 64;
    const long long frame_bits = 9 + (l.segs - 1) * gif_worst_bits(d->segment) + gif_worst_bits(l.pixels - (l.segs - 1) * d->segment);
    l.raw_words = (frame_bits + 31) / 32 + 1;
    const size_t stream = (size_t)((frame_bits + 7) / 8);
    l.head = 13 + 768 + (d->loop >= 0 ? 19 : 0);
    l.file_cap = (size_t)l.head + n * (20 + stream + (stream + 254) / 255) + 1;
    Carve c;
    l.total = c.take(8);                                      // (the file follows at 256: gif_file_at)
    l.file = c.take(l.file_cap);
    l.hist = c.take((size_t)MM_GIF_BINS * 16);
    l.lut = c.take(MM_GIF_BINS);
    l.raw = c.take(n * (size_t)l.raw_words * 4);
    l.seg_bits = c.take(n * (size_t)l.segs * 8);
    l.zero_bytes = l.seg_bits - l.hist;                       // the histogram, the table and the streams start as zeros
    l.frame_len = c.take((2 * n + 1) * 8);                    // where each frame starts (n + 1), then each frame's bits
    l.slots = c.take(n * (size_t)l.segs * l.slot_words * 4);
    l.bytes = c.at;
    return l;
}
size_t gif_workspace_bytes(const MMGifDesc* d) { return d->quantize_only ? 256 + (size_t)MM_GIF_BINS * 17 : gif_layout(d).bytes; }
size_t gif_file_at(const MMGifDesc* d) { (void)d; return 256; }

struct GifArgs {
    const unsigned char* frames; const int* delays;
    unsigned char* palette; unsigned char* indices;
    long long* total; unsigned char* file; unsigned long long* hist; unsigned char* lut; unsigned* raw;
    unsigned long long* seg_bits; long long* frame_len; unsigned* slots;
    int n, H, W, segment, delay, loop, head;
    long long pixels, all_pixels, segs, all_segs, raw_words;
    int slot_words, table_slots, table_shift, group;
};

__device__ inline int gif_bin(const unsigned char* p) { return (p[0] >> 3) << 10 | (p[1] >> 3) << 5 | (p[2] >> 3); }

// a run of one bin's pixels into the histogram: count | sum r&7 << 32, sum g&7 | sum b&7 << 32
__device__ inline void gif_flush(unsigned long long* hist, int bin, unsigned c, unsigned sr, unsigned sg, unsigned sb) {
    atomicAdd(hist + 2 * bin, (unsigned long long)c | (unsigned long long)sr << 32);
    atomicAdd(hist + 2 * bin + 1, (unsigned long long)sg | (unsigned long long)sb << 32);
}

// ---- histogram ------------------------------------------------------------------------------------------------------------------------
// a run into the workgroup's table (bin -> the two sums, open addressing, eight probes), or past a full table straight into the histogram
__device__ inline void gif_gather(unsigned* keys, unsigned long long* vals, unsigned long long* hist, int bin, unsigned c, unsigned sr, unsigned sg, unsigned sb) {
    unsigned h = ((unsigned)bin * 2654435761u) >> (32 - MM_GIF_HIST_LOG2);
    for (int probe = 0; probe < 8; ++probe) {
        const unsigned old = atomicCAS(&keys[h], 0xFFFFFFFFu, (unsigned)bin);
        if (old == 0xFFFFFFFFu || old == (unsigned)bin) {
            atomicAdd(&vals[2 * h], (unsigned long long)c | (unsigned long long)sr << 32);
            atomicAdd(&vals[2 * h + 1], (unsigned long long)sg | (unsigned long long)sb << 32);
            return;
        }
        h = (h + 1) & (MM_GIF_HIST_SLOTS - 1);
    }
    gif_flush(hist, bin, c, sr, sg, sb);
}

__global__ __launch_bounds__(MM_GIF_BLOCK) void gif_histogram_kernel(GifArgs a) {
    __shared__ unsigned keys[MM_GIF_HIST_SLOTS];
    __shared__ unsigned long long vals[2 * MM_GIF_HIST_SLOTS];
    for (int i = threadIdx.x; i < MM_GIF_HIST_SLOTS; i += MM_GIF_BLOCK) { keys[i] = 0xFFFFFFFFu; vals[2 * i] = 0; vals[2 * i + 1] = 0; }
    __syncthreads();
    const long long p0 = ((long long)blockIdx.x * MM_GIF_BLOCK + threadIdx.x) * MM_GIF_RUN;
    const long long p1 = min(p0 + MM_GIF_RUN, a.all_pixels);
    int bin = -1;
    unsigned c = 0, sr = 0, sg = 0, sb = 0;
    for (long long p = p0; p < p1; ++p) {
        const unsigned char* px = a.frames + p * 3;
        const int b = gif_bin(px);
        if (b != bin) {
            if (c) gif_gather(keys, vals, a.hist, bin, c, sr, sg, sb);
            bin = b; c = sr = sg = sb = 0;
        }
        c += 1; sr += px[0] & 7; sg += px[1] & 7; sb += px[2] & 7;
    }
    // the runs still open: those of the first lane's bin leave as one sum (every lane of the wave is here; a lane without pixels has c = 0)
    const int lead = __builtin_amdgcn_readfirstlane(bin);
    const bool same = lead >= 0 && bin == lead;
    int tc, tr, tg, tb;
    (void)wave_prefix_excl(same ? (int)c : 0, 0, tc);
    (void)wave_prefix_excl(same ? (int)sr : 0, 0, tr);
    (void)wave_prefix_excl(same ? (int)sg : 0, 0, tg);
    (void)wave_prefix_excl(same ? (int)sb : 0, 0, tb);
    if ((threadIdx.x & 63) == 0) { if (tc) gif_gather(keys, vals, a.hist, lead, (unsigned)tc, (unsigned)tr, (unsigned)tg, (unsigned)tb); }
    else if (!same && c) gif_gather(keys, vals, a.hist, bin, c, sr, sg, sb);
    __syncthreads();
    for (int i = threadIdx.x; i < MM_GIF_HIST_SLOTS; i += MM_GIF_BLOCK)
        if (keys[i] != 0xFFFFFFFFu) {
            atomicAdd(a.hist + 2 * keys[i], vals[2 * i]);
            atomicAdd(a.hist + 2 * keys[i] + 1, vals[2 * i + 1]);
        }
}

// ---- median cut: one workgroup ----------------------------------------------------------------------------------------------------------
struct GifBox { unsigned count, bins; int lo[3], hi[3]; };   // axis 0 r, 1 g, 2 b

__device__ inline int gif_coord(int bin, int axis) { return (bin >> (10 - 5 * axis)) & 31; }

// what a lane gathers of one box over its own entries before it touches the shared statistics
struct GifAcc {
    unsigned count = 0, bins = 0;
    int lo[3] = {31, 31, 31}, hi[3] = {0, 0, 0};
    __device__ inline void add(int bin, unsigned c) {
        count += c; bins += 1;
#pragma unroll
        for (int x = 0; x < 3; ++x) { lo[x] = min(lo[x], gif_coord(bin, x)); hi[x] = max(hi[x], gif_coord(bin, x)); }
    }
    // every lane of the wave calls it: the wave's sum first, then one lane's atomics
    __device__ inline void into(GifBox& b, int lane) const {
        int c, n;
        (void)wave_prefix_excl((int)count, lane, c);
        (void)wave_prefix_excl((int)bins, lane, n);
        int l[3], h[3];
#pragma unroll
        for (int x = 0; x < 3; ++x) { l[x] = (int)wave_min_u32((unsigned)lo[x]); h[x] = wave_max_i32(hi[x]); }
        if (lane != 0 || n == 0) return;
        atomicAdd(&b.count, (unsigned)c); atomicAdd(&b.bins, (unsigned)n);
#pragma unroll
        for (int x = 0; x < 3; ++x) { atomicMin(&b.lo[x], l[x]); atomicMax(&b.hi[x], h[x]); }
    }
};

__global__ __launch_bounds__(MM_GIF_CUT_BLOCK) void gif_median_cut_kernel(GifArgs a) {
    __shared__ unsigned short ent_bin[MM_GIF_BINS];
    __shared__ GifBox box[256];
    __shared__ unsigned long long sum[256][3];
    __shared__ unsigned best_count, best_box;
    __shared__ unsigned marg[32];
    __shared__ int scan_sh[MM_GIF_CUT_BLOCK / 64];
    __shared__ int cut;
    const int tid = threadIdx.x;
    const unsigned long long* hist = a.hist;

    // the non-empty bins, ascending
    constexpr int PER = MM_GIF_BINS / MM_GIF_CUT_BLOCK;
    int mine = 0;
    for (int j = 0; j < PER; ++j) mine += (unsigned)hist[2 * (tid * PER + j)] != 0u;
    if (tid < 256) {
        box[tid].count = 0; box[tid].bins = 0;
        for (int x = 0; x < 3; ++x) { box[tid].lo[x] = 31; box[tid].hi[x] = 0; sum[tid][x] = 0; }
    }
    int M;
    int at = block_prefix_excl<MM_GIF_CUT_BLOCK>(mine, tid, scan_sh, M);      // (its barriers also publish the boxes)
    for (int j = 0; j < PER; ++j) {
        const int bin = tid * PER + j;
        if ((unsigned)hist[2 * bin] != 0u) ent_bin[at++] = (unsigned short)bin;
    }
    __syncthreads();
    // entry j * 1024 + tid lives in this lane's registers from here on: bin | box << 16 (0xFFFF: no entry) and the bin's pixel count
    unsigned ent[PER], cnt[PER];
    {
        GifAcc acc;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int e = j * MM_GIF_CUT_BLOCK + tid;
            ent[j] = 0xFFFF0000u; cnt[j] = 0;
            if (e < M) { ent[j] = ent_bin[e]; cnt[j] = (unsigned)hist[2 * ent[j]]; acc.add((int)ent[j], cnt[j]); }
        }
        acc.into(box[0], tid & 63);
    }
    int boxes = 1;
    while (boxes < 256) {
        if (tid == 0) { best_count = 0; best_box = 256; }
        if (tid < 32) marg[tid] = 0;
        __syncthreads();                                      // (also: the statistics of the last split are complete)
        const bool splittable = tid < boxes && box[tid].bins >= 2;          // (two bins hold two pixels at least: the count is not 0)
        if (splittable) atomicMax(&best_count, box[tid].count);
        __syncthreads();
        if (splittable && box[tid].count == best_count) atomicMin(&best_box, (unsigned)tid);
        __syncthreads();
        if (best_box == 256) break;                           // (uniform: every lane reads the same word)
        const unsigned target = best_box;
        const int er = box[target].hi[0] - box[target].lo[0], eg = box[target].hi[1] - box[target].lo[1], eb = box[target].hi[2] - box[target].lo[2];
        const int axis = (eg >= er && eg >= eb) ? 1 : (er >= eb ? 0 : 2);
        const int lo = box[target].lo[axis], hi = box[target].hi[axis];
        const unsigned half = (box[target].count + 1) / 2;
#pragma unroll
        for (int j = 0; j < PER; ++j)
            if ((ent[j] >> 16) == target) atomicAdd(&marg[gif_coord((int)(ent[j] & 0xFFFFu), axis)], cnt[j]);
        __syncthreads();
        if (tid == 0) {
            unsigned cum = 0;
            int k = lo;
            for (; k < hi - 1; ++k) { cum += marg[k]; if (cum >= half) break; }
            cut = k;
            for (int b = 0; b < 2; ++b) {
                GifBox& x = box[b ? (unsigned)boxes : target];
                x.count = 0; x.bins = 0;
                for (int c = 0; c < 3; ++c) { x.lo[c] = 31; x.hi[c] = 0; }
            }
        }
        __syncthreads();
        const int k = cut;
        GifAcc stay, go;
#pragma unroll
        for (int j = 0; j < PER; ++j)
            if ((ent[j] >> 16) == target) {
                const int bin = (int)(ent[j] & 0xFFFFu);
                if (gif_coord(bin, axis) > k) { ent[j] = (unsigned)bin | (unsigned)boxes << 16; go.add(bin, cnt[j]); }
                else stay.add(bin, cnt[j]);
            }
        stay.into(box[target], tid & 63);
        go.into(box[boxes], tid & 63);
        ++boxes;
    }
    __syncthreads();
    // the boxes' means and the table
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (ent[j] == 0xFFFF0000u) continue;
        const int bin = (int)(ent[j] & 0xFFFFu), b = (int)(ent[j] >> 16);
        const unsigned long long h0 = hist[2 * bin], h1 = hist[2 * bin + 1];
        const unsigned long long c = h0 & 0xFFFFFFFFull;
        atomicAdd(&sum[b][0], c * (unsigned long long)(gif_coord(bin, 0) << 3) + (h0 >> 32));
        atomicAdd(&sum[b][1], c * (unsigned long long)(gif_coord(bin, 1) << 3) + (h1 & 0xFFFFFFFFull));
        atomicAdd(&sum[b][2], c * (unsigned long long)(gif_coord(bin, 2) << 3) + (h1 >> 32));
        a.lut[bin] = (unsigned char)b;
    }
    __syncthreads();
    if (tid < 256) {
        const unsigned long long c = tid < boxes ? box[tid].count : 0;
        for (int x = 0; x < 3; ++x) a.palette[tid * 3 + x] = c ? (unsigned char)((2 * sum[tid][x] + c) / (2 * c)) : 0;
    }
}

// ---- index: a pixel's box ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_GIF_BLOCK) void gif_index_kernel(GifArgs a) {
    const long long p = (long long)blockIdx.x * MM_GIF_BLOCK + threadIdx.x;
    if (p < a.all_pixels) a.indices[p] = a.lut[gif_bin(a.frames + p * 3)];
}

// ---- code: a lane per segment -----------------------------------------------------------------------------------------------------------
struct GifBits {
    unsigned long long acc = 0;
    int nacc = 0;
    unsigned* out;
    unsigned words = 0;
    __device__ inline void put(unsigned code, int width) {
        acc |= (unsigned long long)code << nacc;
        nacc += width;
        if (nacc >= 32) { out[words++] = (unsigned)acc; acc >>= 32; nacc -= 32; }
    }
    __device__ inline unsigned long long finish() {
        const unsigned long long bits = (unsigned long long)words * 32 + nacc;
        if (nacc > 0) out[words++] = (unsigned)acc;
        return bits;
    }
};

__global__ __launch_bounds__(64) void gif_code_kernel(GifArgs a) {
    extern __shared__ unsigned gif_lds[];
    const int tid = threadIdx.x;
    const int stride = (a.segment + 3) & ~3;
    unsigned* tables = gif_lds;
    unsigned char* pixels = (unsigned char*)(gif_lds + (size_t)a.group * a.table_slots);
    const long long seg0 = (long long)blockIdx.x * a.group;
    const int here = (int)min((long long)a.group, a.all_segs - seg0);
    for (int i = tid; i < here * a.table_slots; i += 64) tables[i] = 0xFFFFFFFFu;
    for (int j = 0; j < here; ++j) {
        const long long seg = seg0 + j, frame = seg / a.segs, s = seg - frame * a.segs;
        const int len = (int)min((long long)a.segment, a.pixels - s * a.segment);
        const unsigned char* src = a.indices + frame * a.pixels + s * a.segment;
        for (int i = tid; i < len; i += 64) pixels[j * stride + i] = src[i];
    }
    __syncthreads();
    if (tid >= here) return;
    const long long seg = seg0 + tid, frame = seg / a.segs, s = seg - frame * a.segs;
    const int len = (int)min((long long)a.segment, a.pixels - s * a.segment);
    const unsigned char* px = pixels + tid * stride;
    unsigned* table = tables + (size_t)tid * a.table_slots;
    const unsigned mask = (unsigned)a.table_slots - 1u;
    GifBits bits;
    bits.out = a.slots + (size_t)seg * a.slot_words;
    if (s == 0) bits.put(256u, 9);
    unsigned next = 258, w = px[0];
    int width = 9;
    for (int i = 1; i < len; ++i) {
        const unsigned c = px[i], key = w << 8 | c;
        unsigned h = (key * 2654435761u) >> a.table_shift;
        unsigned e;
        while ((e = table[h]) != 0xFFFFFFFFu && (e >> 12) != key) h = (h + 1) & mask;
        if (e != 0xFFFFFFFFu) { w = e & 0xFFFu; continue; }
        bits.put(w, width);
        table[h] = key << 12 | next;
        if (next == (1u << width) && width < 12) ++width;
        ++next;
        w = c;
    }
    bits.put(w, width);
    if (next == (1u << width) && width < 12) ++width;
    bits.put(s == a.segs - 1 ? 257u : 256u, width);
    a.seg_bits[seg] = bits.finish();
}

// ---- offsets: per frame, the segments' bit counts -> bit offsets, in place; the frame's length in the file -----------------------------
__global__ __launch_bounds__(MM_GIF_BLOCK) void gif_bit_offsets_kernel(GifArgs a) {
    __shared__ unsigned long long sh[block_scan_words<MM_GIF_BLOCK, unsigned long long>()];
    const int tid = threadIdx.x, frame = blockIdx.x;
    const unsigned long long carry = array_scan<false, MM_GIF_BLOCK>(a.seg_bits + (size_t)frame * a.segs, a.segs, 0ull, tid, sh);
    if (tid == 0) {
        const long long len = (long long)((carry + 7) >> 3);
        a.frame_len[frame + 1] = 20 + len + (len + 254) / 255;
        a.frame_len[a.n + 1 + frame] = (long long)carry;      // (the frame's bits, kept behind the offsets for the pack and write passes)
    }
}

// ---- pack: a segment's words into its frame's stream ------------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_GIF_BLOCK) void gif_pack_kernel(GifArgs a) {
    const long long seg = blockIdx.x;
    const long long frame = seg / a.segs, s = seg - frame * a.segs;
    const unsigned long long off = a.seg_bits[seg];
    const unsigned long long nbits = (s + 1 < a.segs ? a.seg_bits[seg + 1] : (unsigned long long)a.frame_len[a.n + 1 + frame]) - off;
    const int w = blockIdx.y * MM_GIF_BLOCK + threadIdx.x;
    if (w >= a.slot_words || (unsigned long long)w * 32 >= nbits) return;
    const unsigned v = a.slots[(size_t)seg * a.slot_words + w];
    if (!v) return;
    const unsigned long long at = off + (unsigned long long)w * 32;
    unsigned* dst = a.raw + (size_t)frame * a.raw_words + (at >> 5);
    const int sh = (int)(at & 31);
    atomicOr(dst, v << sh);
    if (sh && (v >> (32 - sh))) atomicOr(dst + 1, v >> (32 - sh));
}

// ---- place: the frames' lengths in frame_len[1..n] -> where each starts, frame_len[0..n]; the file's length ---------------------------
__global__ __launch_bounds__(MM_GIF_BLOCK) void gif_place_kernel(GifArgs a) {
    __shared__ long long sh[block_scan_words<MM_GIF_BLOCK, long long>()];
    const int tid = threadIdx.x;
    if (tid == 0) a.frame_len[0] = a.head;
    const long long carry = array_scan<true, MM_GIF_BLOCK>(a.frame_len + 1, a.n, (long long)a.head, tid, sh);
    if (tid == 0) *a.total = carry + 1;
}

// ---- write ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_GIF_BLOCK) void gif_write_kernel(GifArgs a) {
    const int tid = threadIdx.x, frame = blockIdx.y;
    const long long len = (a.frame_len[a.n + 1 + frame] + 7) >> 3;
    unsigned char* dst = a.file + a.frame_len[frame];
    if (blockIdx.x == 0) {
        if (frame == 0) {
            unsigned char* f = a.file;
            for (int i = tid; i < 768; i += MM_GIF_BLOCK) f[13 + i] = a.palette[i];
            if (tid == 0) {
                const unsigned char sig[6] = {'G', 'I', 'F', '8', '9', 'a'};
                for (int i = 0; i < 6; ++i) f[i] = sig[i];
                f[6] = (unsigned char)a.W; f[7] = (unsigned char)(a.W >> 8); f[8] = (unsigned char)a.H; f[9] = (unsigned char)(a.H >> 8);
                f[10] = 0xF7; f[11] = 0; f[12] = 0;
                if (a.loop >= 0) {
                    const unsigned char ext[16] = {0x21, 0xFF, 0x0B, 'N', 'E', 'T', 'S', 'C', 'A', 'P', 'E', '2', '.', '0', 0x03, 0x01};
                    unsigned char* x = f + 13 + 768;
                    for (int i = 0; i < 16; ++i) x[i] = ext[i];
                    x[16] = (unsigned char)a.loop; x[17] = (unsigned char)(a.loop >> 8); x[18] = 0;
                }
            }
        }
        if (tid == 64) {
            const int delay = a.delays ? a.delays[frame] & 0xFFFF : a.delay;
            const unsigned char h[19] = {0x21, 0xF9, 0x04, 0x04, (unsigned char)delay, (unsigned char)(delay >> 8), 0, 0, 0x2C, 0, 0, 0, 0,
                                         (unsigned char)a.W, (unsigned char)(a.W >> 8), (unsigned char)a.H, (unsigned char)(a.H >> 8), 0, 8};
            for (int i = 0; i < 19; ++i) dst[i] = h[i];
            dst[19 + len + (len + 254) / 255] = 0;
            if (frame == a.n - 1) dst[20 + len + (len + 254) / 255] = 0x3B;
        }
    }
    const unsigned char* raw = (const unsigned char*)(a.raw + (size_t)frame * a.raw_words);
    for (long long j = (long long)blockIdx.x * MM_GIF_BLOCK + tid; j < len; j += (long long)gridDim.x * MM_GIF_BLOCK) {
        const long long q = j / 255;
        dst[19 + j + q + 1] = raw[j];
        if (j - q * 255 == 0) dst[19 + j + q] = (unsigned char)min(len - j, 255LL);
    }
}

int launch_gif(const MMGifDesc* d, hipStream_t s) {
    GifArgs a = {};
    unsigned char* ws = (unsigned char*)d->workspace;
    a.frames = d->frames; a.delays = d->delays; a.palette = d->palette; a.indices = d->indices;
    a.n = d->n; a.H = d->H; a.W = d->W; a.segment = d->segment; a.delay = d->delay; a.loop = d->loop;
    a.pixels = (long long)d->H * d->W; a.all_pixels = a.pixels * d->n;
    const dim3 wg(MM_GIF_BLOCK);
    const unsigned per_pixel = (unsigned)((a.all_pixels + MM_GIF_BLOCK - 1) / MM_GIF_BLOCK);
    const unsigned per_run = (unsigned)((a.all_pixels + (long long)MM_GIF_BLOCK * MM_GIF_RUN - 1) / ((long long)MM_GIF_BLOCK * MM_GIF_RUN));
    size_t zero = (size_t)MM_GIF_BINS * 17;
    a.hist = (unsigned long long*)(ws + 256); a.lut = ws + 256 + (size_t)MM_GIF_BINS * 16;
    GifLayout l = {};
    if (!d->quantize_only) {
        l = gif_layout(d);
        a.total = (long long*)(ws + l.total); a.file = ws + l.file; a.hist = (unsigned long long*)(ws + l.hist); a.lut = ws + l.lut;
        a.raw = (unsigned*)(ws + l.raw); a.seg_bits = (unsigned long long*)(ws + l.seg_bits); a.frame_len = (long long*)(ws + l.frame_len);
        a.slots = (unsigned*)(ws + l.slots);
        a.head = l.head; a.segs = l.segs; a.all_segs = l.segs * d->n; a.raw_words = l.raw_words;
        a.slot_words = l.slot_words; a.table_slots = l.table_slots; a.table_shift = l.table_shift; a.group = l.group;
        zero = l.zero_bytes;
    }
    if (hipMemsetAsync(a.hist, 0, zero, s) != hipSuccess) return launch_ok("gif_zero");
    hipLaunchKernelGGL(gif_histogram_kernel, dim3(per_run), wg, 0, s, a);
    hipLaunchKernelGGL(gif_median_cut_kernel, dim3(1), dim3(MM_GIF_CUT_BLOCK), 0, s, a);
    hipLaunchKernelGGL(gif_index_kernel, dim3(per_pixel), wg, 0, s, a);
    if (d->quantize_only) return launch_ok("gif_quantize");
    const size_t lds = (size_t)l.group * (l.table_slots * 4 + ((d->segment + 3) & ~3));
    hipLaunchKernelGGL(gif_code_kernel, dim3((unsigned)((a.all_segs + l.group - 1) / l.group)), dim3(64), lds, s, a);
    hipLaunchKernelGGL(gif_bit_offsets_kernel, dim3((unsigned)d->n), wg, 0, s, a);
    hipLaunchKernelGGL(gif_pack_kernel, dim3((unsigned)a.all_segs, (unsigned)((l.slot_words + MM_GIF_BLOCK - 1) / MM_GIF_BLOCK)), wg, 0, s, a);
    hipLaunchKernelGGL(gif_place_kernel, dim3(1), wg, 0, s, a);
    const long long stream_cap = l.raw_words * 4;
    const unsigned write_x = (unsigned)min((stream_cap + MM_GIF_BLOCK - 1) / MM_GIF_BLOCK, 256LL);
    hipLaunchKernelGGL(gif_write_kernel, dim3(write_x, (unsigned)d->n), wg, 0, s, a);
    return launch_ok("gif");
}

}  // namespace mm
