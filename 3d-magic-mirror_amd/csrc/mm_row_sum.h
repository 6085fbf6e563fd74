// mm_row_sum.h -- the row sum both reducing backwards end with: view_sum_kernel (mm_views.hip) and index_sum_kernel (mm_indexed.hip).
//
// The backward kernels of the render path write PER-IMAGE gradients; those of vertices, textures, lights and bg land in staging areas of the
// caller's workspace, one row per image, and one launch reduces all four:
//     out[j] = ((g[r0][j] + g[r1][j]) + g[r2][j]) + ...          plain fp32 adds over the sum's staged rows, in their order
// (no fma -- both files are compiled without contraction --, no atomics: bitwise reproducible, the bits of the adds written out in torch).
// A pure stream.  A workgroup takes 4 x 256 consecutive 16-byte units of one output row (every wave instruction = 1 KiB contiguous); per unit
// the staged rows are loaded two at a time, so a lane keeps 8 independent 16-byte loads in flight; no LDS, no scratch.  Rows whose length is
// not a multiple of four floats, or whose pointers are not 16-byte aligned (vertices of most templates, lights), take the same loop with
// 4-byte units: they are a thousandth of the bytes.  Measured: profiles/render_views_kernels.md, profiles/render_indexed_kernels.md.
#pragma once
#include "mm_device.h"

namespace mm {

#define MM_RSUM_UNITS 4            // units per lane (256 apart: coalesced per instruction)

// the four tensors of a sum launch, as both kernels' arguments begin
struct RowSumArgs {
    const float* src[4];           // staging: one row of len floats per image
    float* dst[4];                 // the summed rows
    int len[4];                    // floats per row; 0: tensor not present
    int vec[4];                    // 1: len % 4 == 0 and both pointers 16-byte aligned -> float4 units
};

// fills tensor t of `a`; returns the workgroups (chunks of 256 * MM_RSUM_UNITS units) one of its rows takes, 0 for a tensor that is not summed
inline int row_sum_pack(RowSumArgs& a, int t, const float* staging, float* out, int len) {
    const bool on = len > 0 && staging && out;
    a.src[t] = staging; a.dst[t] = out; a.len[t] = on ? len : 0;
    a.vec[t] = on && (len & 3) == 0 && (((uintptr_t)staging | (uintptr_t)out) & 15) == 0;
    if (!on) return 0;
    const int n = a.vec[t] ? len >> 2 : len;
    return (n + 256 * MM_RSUM_UNITS - 1) / (256 * MM_RSUM_UNITS);
}

__device__ inline float rs_add(const float& a, const float& b) { return a + b; }
__device__ inline float4 rs_add(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

__device__ inline void rs_zero(float& a) { a = 0.f; }
__device__ inline void rs_zero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }

// One workgroup's chunk of one output row: units [chunk * 1024, chunk * 1024 + 1024) of `n` units, summed over `cnt` staged rows; staged row m
// starts at src + m * n.  kList = false: the k-th row of the sum is row k (the views of one sample follow each other; cnt >= 1).  kList = true:
// it is row list[k] (workgroup-uniform, like everything read from the list; read two trips ahead), and a sum of no rows exists: it writes zeros.
template <typename T, bool kList>
__device__ inline void row_sum_chunk(const T* __restrict__ src, T* __restrict__ dst, int n, const int* __restrict__ list, int cnt, int chunk) {
    int u[MM_RSUM_UNITS];
    bool ok[MM_RSUM_UNITS];
    T acc[MM_RSUM_UNITS];
    const int first = kList && cnt > 0 ? list[0] : 0;
#pragma unroll
    for (int k = 0; k < MM_RSUM_UNITS; ++k) {
        u[k] = chunk * (256 * MM_RSUM_UNITS) + k * 256 + (int)threadIdx.x;
        ok[k] = u[k] < n;
        u[k] = ok[k] ? u[k] : 0;                                 // (a valid address in every lane; nothing is stored for it)
        if (!kList || cnt > 0) acc[k] = src[(size_t)first * n + u[k]];      // the first row starts the sum: g0, not 0 + g0
        else rs_zero(acc[k]);                                    // no row: zeros
    }
    int m0 = 0, m1 = 0;                                          // the trip's two rows
    if (kList) { m0 = cnt > 1 ? list[1] : 0; m1 = cnt > 2 ? list[2] : m0; }
    for (int v = 1; v < cnt; v += 2) {
        const bool two = v + 1 < cnt;                            // (workgroup-uniform)
        if (!kList) { m0 = v; m1 = two ? v + 1 : v; }
        T r0[MM_RSUM_UNITS], r1[MM_RSUM_UNITS];
#pragma unroll
        for (int k = 0; k < MM_RSUM_UNITS; ++k) {
            r0[k] = src[(size_t)m0 * n + u[k]];
            r1[k] = src[(size_t)m1 * n + u[k]];
        }
        if (kList) {                                             // (the next trip's images: asked for before this trip's rows are waited for)
            m0 = v + 2 < cnt ? list[v + 2] : 0;
            m1 = v + 3 < cnt ? list[v + 3] : m0;
        }
#pragma unroll
        for (int k = 0; k < MM_RSUM_UNITS; ++k) {
            acc[k] = rs_add(acc[k], r0[k]);
            if (two) acc[k] = rs_add(acc[k], r1[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < MM_RSUM_UNITS; ++k)
        if (ok[k]) dst[u[k]] = acc[k];
}

}  // namespace mm
