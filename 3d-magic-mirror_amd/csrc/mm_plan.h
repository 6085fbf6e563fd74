// mm_plan.h -- the plan of the backward's face sweep, shared by the two grids that can carry its workgroups (mm_pixel_bwd.hip, mm_raster.hip).
#pragma once
#include "mm_device.h"

#define MM_PLAN_WGS 4              // plan workgroups per image where faces are many (else one)

namespace mm {

// ---------------------------------------------------------------------------------------------------------------------
// 0. plan of the face sweep (the first MM_PLAN_WGS * B workgroups of pixel_bwd's grid, or -- step mode, where there is no pixel_bwd -- the
//    last ones of raster_fwd's, which needs only the face records; nothing in the pixel pass depends on it and the gather launch behind it
//    finds it done): every face's inflated pixel box cut into chunks of MM_CHUNK_PX pixels, numbered in face
//    order by an exclusive scan of the chunk counts.  Thread t owns the contiguous faces [t*per, (t+1)*per): it adds up their counts, ONE
//    block scan gives its first item, and it numbers its faces' chunks from there.  Should the items run out (more than sixteen screens'
//    worth of box pixels in one image), the image's chunk size doubles until they fit (item_cap >= F, so it ends).  It used to run
//    between the vertex stage and the walk, on the forward's critical path (63 us at 13 776 faces); here it costs the step nothing.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef MM_PLAN_LDS_FACES
#define MM_PLAN_LDS_FACES 14336   // 28 KiB of LDS: five workgroups per CU stay possible
#endif
// (MM_PLAN_WGS workgroups per image where faces are many, else one: each counts every face -- cheap, from LDS -- and writes the items of its share)
// kOffsets: also the offsets of the texture-record lists (pixel_bwd's grid only; step mode places records without them).
// s_wave, s_nch: the workgroup's LDS (MM_PLAN_WGS x 4 ints, MM_PLAN_LDS_FACES shorts) -- the caller's, so that raster_fwd can overlay its stage
template <bool kOffsets, class Args>
__device__ inline void plan_sweep_items(const Args& a, int b, int q, int (*s_wave)[4], unsigned short* s_nch) {
    const int nwg = a.plan_wgs;                                   // 1 or MM_PLAN_WGS
    // the faces' chunk counts at the base chunk size are staged in LDS (2 bytes a face, read once, coalesced, eight loads in flight per
    // thread): with thousands of faces per thread-range the passes below were a chain of dependent trips to memory, one per face.
    // ceil(ceil(n / c) / 2^k) = ceil(n / (c 2^k)): the doubled chunk sizes need nothing else.
    const int tid = threadIdx.x;
    // First (the pixel workgroups behind this one in the grid want it two trips to memory into their lives): where each texture tile's record list
    // starts in the image's packed array = exclusive scan of the forward's per-tile counts.  Stored + 1: the words are zero until now (cleared with
    // the backward's counters), which is how a pixel lane that got there first knows to ask again.
    if constexpr (kOffsets) if (q == 0) {
#ifdef MM_DBG_LATE_TOFF                                         // (test builds: a plan workgroup that gets going ~0.3 ms late -- every pixel lane has given
        for (int i = 0; i < 100; ++i) __builtin_amdgcn_s_sleep(127);   //  up waiting by then and formed its offset itself; the texture gather still finds these)
#endif
        const int nt = a.ntiles_, per4 = (nt + 255) >> 8, t0 = tid * per4;
        const int* cnt = a.trcnt + (size_t)b * nt;
        int mine = 0;
        for (int i = 0; i < per4; ++i) mine += t0 + i < nt ? cnt[t0 + i] : 0;
        int tot;
        int run = wave_prefix_excl(mine, tid & 63, tot);
        if ((tid & 63) == 0) s_wave[0][tid >> 6] = tot;
        __syncthreads();
        for (int w2 = 0; w2 < (tid >> 6); ++w2) run += s_wave[0][w2];
        for (int i = 0; i < per4; ++i) {
            if (t0 + i < nt) {
                __hip_atomic_store(a.toff + (size_t)b * nt + t0 + i, run + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                run += cnt[t0 + i];
            }
        }
        __syncthreads();                                         // (s_wave is used again below)
    }
    const bool staged = a.F <= MM_PLAN_LDS_FACES;                 // (more faces than that: the counts are re-read from the face records)
    auto box_px = [&](int f) {                                   // pixels of the face's sweep box; 0: the box misses the image, or no pixel refers to the face
        const float4 q2 = a.geo[((size_t)b * a.F + f) * 3 + 2];   //  (most faces of a fine, overlapping mesh: nothing to sweep)
        int own = 1, taken = 1;
        if (a.fflag) { const int2 fl = reinterpret_cast<const int2*>(a.fflag)[(size_t)b * a.F + f]; own = fl.x; taken = fl.y; }
        if (!(own | taken)) return 0;
        int px0, py0, bw, bh;
        sweep_box(__float_as_uint(q2.z), __float_as_uint(q2.w), taken != 0, a.sweep_sx, a.sweep_sy, a.W, a.H, px0, py0, bw, bh);
        return bw * bh;
    };
    if (staged) {
        for (int f0 = tid; f0 < a.F; f0 += 8 * 256) {
            int px[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) px[u] = f0 + u * 256 < a.F ? box_px(f0 + u * 256) : 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) if (f0 + u * 256 < a.F) s_nch[f0 + u * 256] = (unsigned short)min((px[u] + MM_CHUNK_PX - 1) / MM_CHUNK_PX, 65535);
        }
        __syncthreads();
    }
    auto chunks = [&](int f, int shift) {                        // the face's items at chunk size MM_CHUNK_PX << shift
        if (staged) return ((int)s_nch[f] + (1 << shift) - 1) >> shift;
        const int chunk = MM_CHUNK_PX << shift;
        return (box_px(f) + chunk - 1) / chunk;
    };
    // the faces are cut into MM_PLAN_WGS * 256 contiguous ranges; range (k, t) = faces of thread t of workgroup k.  Every workgroup
    // counts all of them (so that it knows the total and what lies in front of its own quarter) and writes only its own.
    const int per = (a.F + nwg * 256 - 1) / (nwg * 256);
    int shift = 0, first = 0, total = 0;
    for (;; ++shift) {
        int mine[MM_PLAN_WGS], pre = 0;
#pragma unroll
        for (int k = 0; k < MM_PLAN_WGS; ++k) {
            if (k >= nwg) { if ((tid & 63) == 63) s_wave[k][tid >> 6] = 0; continue; }      // (workgroup-uniform)
            const int f0 = min(a.F, (k * 256 + tid) * per), f1 = min(a.F, f0 + per);
            mine[k] = 0;
            for (int f = f0; f < f1; ++f) mine[k] += chunks(f, shift);
            int wsum;
            const int inc = wave_prefix_excl(mine[k], tid & 63, wsum) + mine[k];
            if (k == q) pre = inc - mine[k];
            if (k == 0) __syncthreads();                         // (s_wave of the previous round has been read)
            if ((tid & 63) == 63) s_wave[k][tid >> 6] = inc;
        }
        __syncthreads();
        first = pre; total = 0;
#pragma unroll
        for (int k = 0; k < MM_PLAN_WGS; ++k) {
            const int tk = ((s_wave[k][0] + s_wave[k][1]) + s_wave[k][2]) + s_wave[k][3];
            if (k < q) first += tk;
            if (k == q) for (int w = 0; w < (tid >> 6); ++w) first += s_wave[k][w];
            total += tk;
        }
        if (total <= a.item_cap || shift >= 20) break;           // workgroup-uniform (and the same in the image's other workgroups)
    }
    const int chunk = MM_CHUNK_PX << shift;
    const int f0 = min(a.F, (q * 256 + tid) * per), f1 = min(a.F, f0 + per);
    for (int f = f0; f < f1; ++f) {
        const int nch = chunks(f, shift);
        a.plan_chunkmap[(size_t)b * a.F + f] = make_int2(first, nch);
        for (int c = 0; c < nch; ++c) a.plan_items[(size_t)b * a.item_cap + first + c] = make_int2(f, c);
        first += nch;
    }
    if (q == 0 && tid == 0) a.plan_nitems[b] = make_int2(total, chunk);
}

}  // namespace mm
