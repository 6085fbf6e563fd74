// mm_views.hip -- the view sum of a multi-view render's backward (mm_render_views_backward, include/mm_render.h) for gfx950.
//
// The backward kernels of the render path write PER-IMAGE gradients; in a call of B samples x N views those of the four per-sample inputs
// (vertices, textures, lights, bg) land in staging areas of the caller's workspace, shaped (B, N, row), and ONE launch of the kernel below
// reduces all four to (B, row):
//     out[b][j] = ((g[b][0][j] + g[b][1][j]) + g[b][2][j]) + ...          plain fp32 adds in ascending view order
// (no fma -- the file is compiled without contraction --, no atomics: bitwise reproducible, and the same bits as the adds written out in torch).
//
// A pure stream: (N + 1) x the shared tensors' bytes cross the memory bus once.  A workgroup takes 4 x 256 consecutive 16-byte units of one
// sample's row (every wave instruction = 1 KiB contiguous); per unit the views are loaded two at a time, so a lane keeps 8 independent 16-byte
// loads in flight; no LDS, no scratch, 66 VGPRs by the compiler's resource report (-Rpass-analysis=kernel-resource-usage): 7 waves per
// SIMD.  Measured at config 2: 0.85 - 1.03 of the rate of a device-to-device copy of the same bytes (profiles/render_views_kernels.md).
// Rows whose length is not a multiple of four floats (vertices of most templates, lights) take the same loop with 4-byte units: they are
// a thousandth of the bytes.
#include "mm_device.h"

namespace mm {

#define MM_VSUM_UNITS 4            // units per lane (256 apart: coalesced per instruction)

struct ViewSumArgs {
    const float* src[4];           // (B, views, len) staging
    float* dst[4];                 // (B, len)
    int len[4];                    // floats per row; 0: tensor not present
    int vec[4];                    // 1: len % 4 == 0 and both pointers 16-byte aligned -> float4 units
    int xb[5];                     // tensor t owns x-blocks [xb[t], xb[t+1]) of the grid
    int views;
};

template <typename T>
__device__ inline T vs_add(const T& a, const T& b);
template <>
__device__ inline float vs_add<float>(const float& a, const float& b) { return a + b; }
template <>
__device__ inline float4 vs_add<float4>(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// one workgroup's chunk of one sample's row: units [chunk * 1024, chunk * 1024 + 1024) of `n` units; view v of the row starts at src + v * n
template <typename T>
__device__ inline void view_sum_chunk(const T* __restrict__ src, T* __restrict__ dst, int n, int views, int chunk) {
    int u[MM_VSUM_UNITS];
    bool ok[MM_VSUM_UNITS];
    T acc[MM_VSUM_UNITS];
#pragma unroll
    for (int k = 0; k < MM_VSUM_UNITS; ++k) {
        u[k] = chunk * (256 * MM_VSUM_UNITS) + k * 256 + (int)threadIdx.x;
        ok[k] = u[k] < n;
        u[k] = ok[k] ? u[k] : 0;                                 // (a valid address in every lane; nothing is stored for it)
        acc[k] = src[u[k]];                                      // view 0 starts the sum: g0, not 0 + g0
    }
    for (int v = 1; v < views; v += 2) {
        const bool two = v + 1 < views;                          // (workgroup-uniform)
        T r0[MM_VSUM_UNITS], r1[MM_VSUM_UNITS];
#pragma unroll
        for (int k = 0; k < MM_VSUM_UNITS; ++k) {
            r0[k] = src[(size_t)v * n + u[k]];
            r1[k] = src[(size_t)(two ? v + 1 : v) * n + u[k]];
        }
#pragma unroll
        for (int k = 0; k < MM_VSUM_UNITS; ++k) {
            acc[k] = vs_add(acc[k], r0[k]);
            if (two) acc[k] = vs_add(acc[k], r1[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < MM_VSUM_UNITS; ++k)
        if (ok[k]) dst[u[k]] = acc[k];
}

// grid (x-blocks of all four tensors, B samples)
__global__ __launch_bounds__(256) void view_sum_kernel(ViewSumArgs a) {
    const int b = blockIdx.y, x = blockIdx.x;
    const int t = x < a.xb[1] ? 0 : (x < a.xb[2] ? 1 : (x < a.xb[3] ? 2 : 3));   // (workgroup-uniform)
    const int len = a.len[t], chunk = x - a.xb[t];
    const float* src = a.src[t] + (size_t)b * a.views * len;
    float* dst = a.dst[t] + (size_t)b * len;
    if (a.vec[t]) view_sum_chunk<float4>((const float4*)src, (float4*)dst, len >> 2, a.views, chunk);
    else view_sum_chunk<float>(src, dst, len, a.views, chunk);
}

// staging[t] (B, views, len[t]) -> out[t] (B, len[t]) for the tensors with len[t] > 0, one launch.  B <= 65535 (the grid's y dimension).
int launch_view_sum(int B, int views, const float* const* staging, float* const* out, const int* len, hipStream_t s) {
    ViewSumArgs a;
    a.views = views;
    int x = 0;
    for (int t = 0; t < 4; ++t) {
        const bool on = len[t] > 0 && staging[t] && out[t];
        a.src[t] = staging[t]; a.dst[t] = out[t]; a.len[t] = on ? len[t] : 0;
        a.vec[t] = on && (len[t] & 3) == 0 && (((uintptr_t)staging[t] | (uintptr_t)out[t]) & 15) == 0;
        a.xb[t] = x;
        if (on) { const int n = a.vec[t] ? len[t] >> 2 : len[t]; x += (n + 256 * MM_VSUM_UNITS - 1) / (256 * MM_VSUM_UNITS); }
    }
    a.xb[4] = x;
    if (x == 0) return MM_OK;
    hipLaunchKernelGGL(view_sum_kernel, dim3(x, B), dim3(256), 0, s, a);
    return launch_ok("view_sum");
}

}  // namespace mm
