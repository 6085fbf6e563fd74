// mm_stream.h -- what the frame ENCODERS share (mm_jpeg.hip, mm_gif.hip, mm_png.hip), the counterpart of mm_frame.h for the frame makers: an array
// longer than a workgroup turned into its prefix sums, and the host's carve of a workspace.  mm_interp.hip borrows the workgroup scan.
// Every scan here runs in one workgroup per frame or per call, between the passes that do the work: none is worth another algorithm.
// What the encoders do NOT share: their bit sinks (GifBits, and PngBits after it: LSB first, a private slot, plain stores; JpegWriter: MSB first, a shared
// stream, atomic OR on a block's first and last word), their pack kernels, and byte stuffing against sub-blocks.  Those differ in substance.
#pragma once
#include "mm_device.h"

namespace mm {

// words of LDS block_scan_excl wants for a workgroup of NT lanes
template <int NT, class T>
constexpr int block_scan_words() { return sizeof(T) == 4 ? NT / MM_WAVE : NT; }

// Exclusive prefix sum of v over the workgroup of NT lanes, the total in every lane.  Integer T of 32 bits: block_prefix_excl (mm_device.h),
// the DPP wave scan plus the waves' totals.  Of 64 bits: Hillis-Steele in LDS.  Every lane of the workgroup calls it; sh
// (block_scan_words<NT, T>() words) may still be read from the call before.
template <int NT, class T>
__device__ inline T block_scan_excl(T v, int tid, T* sh, T& total) {
    if constexpr (sizeof(T) == 4) {
        int t;
        const int e = block_prefix_excl<NT>((int)v, tid, (int*)sh, t);
        total = (T)t;
        return (T)e;
    } else {
        __syncthreads();
        sh[tid] = v;
        __syncthreads();
        for (int o = 1; o < NT; o <<= 1) {
            const T t = tid >= o ? sh[tid - o] : 0;
            __syncthreads();
            sh[tid] += t;
            __syncthreads();
        }
        total = sh[NT - 1];
        return sh[tid] - v;
    }
}

// THE loop: a[0..n) becomes its prefix sums in place, NT elements a pass behind a running carry that starts at `carry`:
// a[i] = carry + a[0] + ... + a[i-1], plus a[i] itself if INCL.  Returns carry + the sum of the array, in every lane.  One workgroup of NT
// lanes, every lane calls it; the sums are formed in S (wrapping, like the counts they add up), sh as block_scan_excl wants it.
template <bool INCL, int NT, class S, class T>
__device__ inline S array_scan(T* a, long long n, S carry, int tid, S* sh) {
    for (long long base = 0; base < n; base += NT) {
        const long long i = base + tid;
        const S v = i < n ? (S)a[i] : 0;
        S total;
        const S e = block_scan_excl<NT>(v, tid, sh, total);
        if (i < n) a[i] = (T)(carry + e + (INCL ? v : 0));
        carry += total;
    }
    return carry;
}

// the host's carve of a workspace: take(bytes) is where the next array starts, every array on a multiple of 256; `at` ends as the size
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at += align256(bytes); return o; }
};

}  // namespace mm
