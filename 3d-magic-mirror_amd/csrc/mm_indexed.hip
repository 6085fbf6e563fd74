// mm_indexed.hip -- the two kernels an indexed render (mm_render_indexed_*, include/mm_render.h) adds to the render path, for gfx950:
//
//   index_plan_kernel   first launch of the forward.  Image i of the call reads row index[t][i] of tensor t (vertices, textures, lights,
//                       bg).  One workgroup per tensor writes (a) the SANITISED table (M) -- the only table any later kernel reads: an entry
//                       outside [0, rows) becomes 0, is counted into the status word and marks its image bad -- and (b) the backward's CSR:
//                       offsets (rows + 1) and the rows' images (M) in ASCENDING image order, bad images left out.  A stable counting sort:
//                       integer atomics count the rows, a workgroup scan turns the counts into offsets, and the fill walks the images in
//                       chunks of 256 with the chunk's keys in LDS: a lane finds its rank among the chunk's earlier equal keys there, the
//                       first lane of every key takes the key's places of the chunk from the row's cursor (one returning integer atomic)
//                       and the chunks follow each other behind a barrier -- so a row's list is ascending whatever the atomics' order.
//                       Counters and cursors of up to 8192 rows live in LDS, more rows use the workspace's (a sheet's 1764 images
//                       count into 7 rows: with every counter in memory the kernel took 90 us, with LDS counters 73-75 us; at M = 96
//                       over 48 rows 16 against 13 us: profiles/render_indexed_kernels.md).  What remains is one workgroup's chain of
//                       barriers, index loads and the 256-key rank scan per chunk, not profiled further.  No host synchronisation,
//                       nothing read back.
//   index_sum_kernel    last launch of the backward.  The backward kernels write PER-IMAGE gradients; those of the four indexed inputs land
//                       in staging areas (M, row) of the workspace, and this launch reduces all four to (rows, row) with the row sum of
//                       mm_row_sum.h: a row's staged rows are those of its list's images, in the list's order; an empty list writes
//                       zeros.  The grid's last workgroups write NaN into the four camera gradients of bad images.
#include "mm_row_sum.h"

namespace mm {

struct IndexPlanArgs {
    const int32_t* index[4];       // (M) the caller's indices; nullptr: the identity
    int rows[4];
    int M;
    int* table;                    // (5, M): the sanitised rows of tensors 0..3, then the images' bad flags (index_row, mm_device.h)
    int* offsets[4];               // (rows + 1)
    int* cursor[4];                // (rows) the rows' counts, then their fill cursors
    int* images[4];                // (M)
    int32_t* status;               // the caller's status word (device or pinned host memory) or nullptr
};

#define MM_IX_NONE 0xFFFFu         // LDS key of a lane without an image to place (rows <= 65535: no row has it)

__device__ inline int plan_key(const IndexPlanArgs& a, int t, int i, bool& bad) {
    const int k = a.index[t] ? a.index[t][i] : i;
    bad = k < 0 || k >= a.rows[t];
    return bad ? 0 : k;
}
__device__ inline bool plan_image_bad(const IndexPlanArgs& a, int i) {
    bool any = false;
#pragma unroll
    for (int t = 0; t < 4; ++t) { bool bad; (void)plan_key(a, t, i, bad); any = any || bad; }
    return any;
}

#define MM_IX_LDS_ROWS 8192        // row counts up to this keep their counters and cursors in LDS (32 KB); larger ones in the workspace

// counters / cursors of the rows: LDS words where the rows fit (no trip to memory in the count, the scan or the fill), else the workspace's
template <bool kLds>
__device__ inline void cur_add(int* cur, int k, int v) {
    if (kLds) __hip_atomic_fetch_add(cur + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else atomicAdd(cur + k, v);
}
template <bool kLds>
__device__ inline int cur_take(int* cur, int k, int v) {
    return kLds ? __hip_atomic_fetch_add(cur + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : atomicAdd(cur + k, v);
}
template <bool kLds>
__device__ inline int cur_load(int* cur, int k) {
    return kLds ? cur[k] : __hip_atomic_load(cur + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool kLds>
__device__ inline void cur_sync() {                              // the workgroup's counter updates are visible to all of it
    if (!kLds) __threadfence();
    __syncthreads();
}

// this lane's key of image i in the fill: its row, or MM_IX_NONE for no image / a bad one
__device__ inline unsigned fill_key(const IndexPlanArgs& a, int t, int i) {
    if (i >= a.M || plan_image_bad(a, i)) return MM_IX_NONE;
    bool bad;
    return (unsigned)plan_key(a, t, i, bad);
}

template <bool kLds>
__device__ inline void index_plan(const IndexPlanArgs& a, int t, int* cur, unsigned short* s_key, int* s_base, int* s_wave) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.rows[t], M = a.M;
    int* offsets = a.offsets[t];
    int* images = a.images[t];
    for (int r = tid; r < R; r += 256) cur[r] = 0;
    cur_sync<kLds>();
    // ---- the table, the bad flags, the rows' counts: four images per lane and trip, their sixteen index loads in flight together
    int nbad = 0;
    for (int i0 = 0; i0 < M; i0 += 1024) {
        int k[4]; bool bad[4], any[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = min(i0 + q * 256 + tid, M - 1);        // (a valid image in every lane; nothing is written for a repeated one)
            k[q] = plan_key(a, t, i, bad[q]);
            any[q] = plan_image_bad(a, i);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * 256 + tid;
            if (i >= M) continue;
            a.table[(size_t)t * M + i] = k[q];
            if (t == 0) a.table[(size_t)4 * M + i] = any[q] ? 1 : 0;
            nbad += bad[q] ? 1 : 0;
            if (!any[q]) cur_add<kLds>(cur, k[q], 1);
        }
    }
    if (a.status) {
        int total;
        (void)wave_prefix_excl(nbad, lane, total);
        if (lane == 0 && total != 0) __hip_atomic_fetch_add(a.status, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (the host may be polling it)
    }
    cur_sync<kLds>();
    // ---- counts -> offsets (exclusive scan, 256 rows per trip); the cursors start at the offsets
    int running = 0;
    for (int r0 = 0; r0 < R; r0 += 256) {
        const int r = r0 + tid;
        const int c = r < R ? cur_load<kLds>(cur, r) : 0;
        int total;
        const int excl = wave_prefix_excl(c, lane, total);
        if (lane == 0) s_wave[wave] = total;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { before += w < wave ? s_wave[w] : 0; all += s_wave[w]; }
        if (r < R) { offsets[r] = running + before + excl; cur[r] = running + before + excl; }
        running += all;
        __syncthreads();
    }
    if (tid == 0) offsets[R] = running;
    cur_sync<kLds>();
    // ---- the stable fill, a chunk of 256 images per trip (the next chunk's indices are asked for before this chunk is placed)
    unsigned key = fill_key(a, t, tid);
    for (int i0 = 0; i0 < M; i0 += 256) {
        const int i = i0 + tid;
        const unsigned next = fill_key(a, t, i + 256);
        s_key[tid] = (unsigned short)key;
        __syncthreads();
        int rank = 0, total = 0, first = -1;                     // equal keys in front of this lane / in the chunk; the chunk's first lane with the key
        for (int q = 0; q < 32; ++q) {                           // (every lane reads the same 16 bytes: an LDS broadcast)
            const uint4 kk = reinterpret_cast<const uint4*>(s_key)[q];
            const unsigned w4[4] = {kk.x, kk.y, kk.z, kk.w};
#pragma unroll
            for (int h = 0; h < 8; ++h) {
                const unsigned kj = (w4[h >> 1] >> ((h & 1) * 16)) & 0xFFFFu;
                const int j = q * 8 + h;
                const bool eq = kj == key;
                total += eq ? 1 : 0;
                rank += (eq && j < tid) ? 1 : 0;
                first = (eq && first < 0) ? j : first;
            }
        }
        if (key != MM_IX_NONE && first == tid) s_base[tid] = cur_take<kLds>(cur, (int)key, total);
        __syncthreads();
        if (key != MM_IX_NONE) images[s_base[first] + rank] = i;
        __syncthreads();                                         // (the chunk's places are taken: the next chunk's follow them)
        key = next;
    }
}

// grid (4): one workgroup per tensor
__global__ __launch_bounds__(256) void index_plan_kernel(IndexPlanArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned short s_key[256];
    __shared__ int s_base[256];
    __shared__ int s_wave[4];
    __shared__ int s_cur[MM_IX_LDS_ROWS];
    const int t = blockIdx.x;
    if (a.rows[t] <= MM_IX_LDS_ROWS) index_plan<true>(a, t, s_cur, s_key, s_base, s_wave);      // (workgroup-uniform)
    else index_plan<false>(a, t, a.cursor[t], s_key, s_base, s_wave);
}

int launch_index_plan(int M, const int32_t* const* index, const int* rows, const IndexPlan& p, int32_t* status, hipStream_t s) {
    IndexPlanArgs a;
    a.M = M; a.table = p.table; a.status = status;
    for (int t = 0; t < 4; ++t) { a.index[t] = index[t]; a.rows[t] = rows[t]; a.offsets[t] = p.offsets[t]; a.cursor[t] = p.cursor[t]; a.images[t] = p.images[t]; }
    hipLaunchKernelGGL(index_plan_kernel, dim3(4), dim3(256), 0, s, a);
    return launch_ok("index_plan");
}

// ---- the index sum -------------------------------------------------------------------------------------------------------------------
struct IndexSumArgs {
    RowSumArgs t;                  // src (M, len), dst (rows, len)
    int cpr[4];                    // workgroups (chunks of 1024 units) per row
    int xb[5];                     // tensor t owns blocks [xb[t], xb[t+1]) of the grid, rows[t] x cpr[t] of them; the blocks from xb[4] on poison the bad images' camera gradients
    const int* offsets[4];
    const int* images[4];
    const int* bad;                // (M)
    int M;
    float *grad_azim, *grad_elev, *grad_dist, *grad_bias;
};

// grid: per tensor rows x chunks-per-row workgroups, row-major -- every tensor has its own row extent, no workgroup is launched for a row a
// tensor does not have --, then the bad images' blocks
__global__ __launch_bounds__(256) void index_sum_kernel(IndexSumArgs a) {
    const int x = blockIdx.x;
    if (x >= a.xb[4]) {                                          // (workgroup-uniform)
        const int i = (x - a.xb[4]) * 256 + (int)threadIdx.x;
        if (i >= a.M || !a.bad[i]) return;
        const float nan = __uint_as_float(0x7FC00000u);
        a.grad_azim[i] = nan; a.grad_elev[i] = nan; a.grad_dist[i] = nan; a.grad_bias[2 * i] = nan; a.grad_bias[2 * i + 1] = nan;
        return;
    }
    const int t = x < a.xb[1] ? 0 : (x < a.xb[2] ? 1 : (x < a.xb[3] ? 2 : 3));   // (workgroup-uniform)
    const int len = a.t.len[t], r = (x - a.xb[t]) / a.cpr[t], chunk = (x - a.xb[t]) % a.cpr[t];
    const int beg = a.offsets[t][r], cnt = a.offsets[t][r + 1] - beg;
    const int* list = a.images[t] + beg;
    float* dst = a.t.dst[t] + (size_t)r * len;
    if (a.t.vec[t]) row_sum_chunk<float4, true>((const float4*)a.t.src[t], (float4*)dst, len >> 2, list, cnt, chunk);
    else row_sum_chunk<float, true>(a.t.src[t], dst, len, list, cnt, chunk);
}

// staging[t] (M, len[t]) -> out[t] (rows[t], len[t]) for the tensors with len[t] > 0, and NaN into the camera gradients of bad images: one launch.
int launch_index_sum(int M, const int* rows, const float* const* staging, float* const* out, const int* len, const IndexPlan& p,
                     const MMRenderGrads* g, hipStream_t s) {
    IndexSumArgs a;
    a.M = M; a.bad = p.table + (size_t)4 * M;
    a.grad_azim = g->grad_azimuths; a.grad_elev = g->grad_elevations; a.grad_dist = g->grad_distances; a.grad_bias = g->grad_biases;
    long long x = 0;
    for (int t = 0; t < 4; ++t) {
        a.offsets[t] = p.offsets[t]; a.images[t] = p.images[t];
        a.xb[t] = (int)x;
        const int cpr = row_sum_pack(a.t, t, staging[t], out[t], len[t]);
        a.cpr[t] = cpr ? cpr : 1;
        x += (long long)rows[t] * cpr;
        if (x > 0x7fff0000LL) return MM_ERR_UNSUPPORTED;          // (65535 rows of a 16-megapixel background: not a render)
    }
    a.xb[4] = (int)x;
    x += (M + 255) / 256;
    hipLaunchKernelGGL(index_sum_kernel, dim3((unsigned)x), dim3(256), 0, s, a);
    return launch_ok("index_sum");
}

}  // namespace mm
