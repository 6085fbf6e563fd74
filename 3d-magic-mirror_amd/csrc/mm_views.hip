// mm_views.hip -- the view sum of a multi-view render's backward (mm_render_views_backward, include/mm_render.h) for gfx950: the staging areas
// (B, N, row) of the per-image gradients of vertices, textures, lights and bg reduced to (B, row) in ascending view order by ONE launch of the
// row sum of mm_row_sum.h.  (N + 1) x the shared tensors' bytes cross the memory bus once; 66 VGPRs by the compiler's resource report
// (-Rpass-analysis=kernel-resource-usage): 7 waves per SIMD.  Measured at config 2: 0.85 - 1.03 of the rate of a device-to-device copy of the
// same bytes (profiles/render_views_kernels.md).
#include "mm_row_sum.h"

namespace mm {

struct ViewSumArgs {
    RowSumArgs t;                  // src (B, views, len), dst (B, len)
    int xb[5];                     // tensor t owns x-blocks [xb[t], xb[t+1]) of the grid
    int views;
};

// grid (x-blocks of all four tensors, B samples)
__global__ __launch_bounds__(256) void view_sum_kernel(ViewSumArgs a) {
    const int b = blockIdx.y, x = blockIdx.x;
    const int t = x < a.xb[1] ? 0 : (x < a.xb[2] ? 1 : (x < a.xb[3] ? 2 : 3));   // (workgroup-uniform)
    const int len = a.t.len[t], chunk = x - a.xb[t];
    const float* src = a.t.src[t] + (size_t)b * a.views * len;
    float* dst = a.t.dst[t] + (size_t)b * len;
    if (a.t.vec[t]) row_sum_chunk<float4, false>((const float4*)src, (float4*)dst, len >> 2, nullptr, a.views, chunk);
    else row_sum_chunk<float, false>(src, dst, len, nullptr, a.views, chunk);
}

// staging[t] (B, views, len[t]) -> out[t] (B, len[t]) for the tensors with len[t] > 0, one launch.  B <= 65535 (the grid's y dimension).
int launch_view_sum(int B, int views, const float* const* staging, float* const* out, const int* len, hipStream_t s) {
    ViewSumArgs a;
    a.views = views;
    int x = 0;
    for (int t = 0; t < 4; ++t) { a.xb[t] = x; x += row_sum_pack(a.t, t, staging[t], out[t], len[t]); }
    a.xb[4] = x;
    if (x == 0) return MM_OK;
    hipLaunchKernelGGL(view_sum_kernel, dim3(x, B), dim3(256), 0, s, a);
    return launch_ok("view_sum");
}

}  // namespace mm
