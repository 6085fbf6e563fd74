// mm_vertex.hip -- vertex stage of the render path (forward and backward) for gfx950.
//
// Forward  (replaces smr_utils camera math + kaolin prepare_vertices + face_normals, networks.py:278-295):
//   one thread per (image, face): camera transform (built once per workgroup), 3 vertex transforms, perspective
//   divide, x multiplier, inflated pixel box, unit normal.  Writes the packed face records the pixel stage streams plus
//   attributes['face_normals'], and -- the 64 faces of a wave being exactly one word of the screen-bin candidate mask --
//   that mask: per block of 8x8 bins one wave transpose of the lanes' coverage bits (no separate binning pass).
//   Small screens and meshes: one more workgroup per image sorts the image's tiles for the walk, from boxes it forms itself (order_workgroup).
// Backward (reverse of the above): one workgroup per image walks the static vertex->corner CSR, so per-vertex
//   gradients are gathered in a fixed order (no atomics), reduces dT in LDS and finishes with the camera chain.
//
// This file is compiled TWICE: on its own (the kernels mm_render_forward / mm_render_backward launch), and once more through
// mm_vertex_views.hip with MM_VERTEX_VIEWS defined -- the same kernels under the names *_views, in which image b reads the vertices of
// SAMPLE b / views (multi-view calls, mm_render_views_*: `vertices` holds B / views rows).  A second compilation instead of a template
// parameter: the first one then sees unchanged tokens, and its kernels keep their symbols and their machine code to the instruction
// (tools/kernel_disasm_diff.py).  And a THIRD time through mm_vertex_indexed.hip with MM_VERTEX_INDEXED defined -- the names *_indexed, in which
// image b reads the vertices of row vrow[b], the plan's sanitised table (indexed calls, mm_render_indexed_*); only that compilation's argument
// structs carry the table's pointer, and its launchers take it in the place of the view count.
#include "mm_device.h"
#if !defined(MM_VERTEX_INDEXED) && !defined(MM_VERTEX_VIEWS)
#include "mm_order.h"
#define MM_VX_ORDER 1         // this compilation's forward kernel carries the order workgroups (below); the other two keep their code
#endif

#if defined(MM_VERTEX_INDEXED)
#define MM_VX(name) name##_indexed
#define MM_VX_SAMPLE(b) (a.vrow[b])
#define MM_VX_PARAM const int* vrow
#define MM_VX_SET(a) do { (a).views = 1; (a).vrow = vrow; } while (0)
#define MM_VX_ONE_VIEW true
#elif defined(MM_VERTEX_VIEWS)
#define MM_VX(name) name##_views
#define MM_VX_SAMPLE(b) ((b) / a.views)
#define MM_VX_PARAM int views
#define MM_VX_SET(a) (a).views = views
#define MM_VX_ONE_VIEW (views == 1)
#else
#define MM_VX(name) name
#define MM_VX_SAMPLE(b) (b)
#define MM_VX_PARAM int views
#define MM_VX_SET(a) (a).views = views
#define MM_VX_ONE_VIEW (views == 1)
#endif

namespace mm {

struct VertexFwdArgs {
    int B, V, F, H, W;
    float proj0, proj1, proj2, mult, infl;
    const int32_t* faces;
    const float* vertices;
    const float *azim, *elev, *dist, *bias;
    float* T;
    float* cam;
    float4* geo;
    float* face_normals;
    int* tcnt; int ntcnt;    // texture-record counters of the backward: cleared here for the first backward after this forward
    int views;               // images per sample (read by the *_views kernels only; it sits in what was padding: no other member moves)
    long long* ltot; int nltot;   // fused-loss sums of the raster waves: cleared here
    int bin_shift, nbx, nby, words;
    uint64_t* mask;          // (B,nbins,words) screen-bin candidate mask, written here (nullptr: not wanted)
    int* fflag;              // (B,F) "this face receives gradient from the pixels": cleared here, set by raster_fwd
    unsigned* ticket;        // (B) arrival counter of the vertex backward's workgroups: cleared here (and by its last workgroup after use)
#ifdef MM_VERTEX_INDEXED
    const int* vrow;         // (B) the row of `vertices` every image reads
#endif
#ifdef MM_VX_ORDER
    // the order workgroups (order_rows > 0: the grid's first order_rows rows, gridDim.x images each): the images' tile orders
    unsigned short* order;   // (B,4*blocks_per_image)
    int* nheavy;             // (B,4)
    int order_rows, blocks_x, blocks_per_image;
#endif
};

__device__ inline void block_camera(const float* azim, const float* elev, const float* dist, const float* bias, int b,
                                    float* s_trig, Camera* s_cam) {
    const int tid = threadIdx.x;
    if (tid < 4) {
        const float ang = MM_DEG2RAD * (tid < 2 ? elev[b] : azim[b]);
        // fp64 sin/cos rounded to fp32: the oracle does the same, so both sides see correctly rounded values
        s_trig[tid] = (tid & 1) ? (float)sin((double)ang) : (float)cos((double)ang);
    }
    __syncthreads();
    if (tid == 0) camera_build(dist[b], s_trig[0], s_trig[1], s_trig[2], s_trig[3], bias[2 * b], bias[2 * b + 1], *s_cam);
    __syncthreads();
}

// one face's positions: camera transform of its three vertices, perspective divide, x multiplier -> its screen corners, and their pixel box
// inflated by the soft-mask margin.  ONE text for the record path and for the order workgroups, which repeat it to count the tiles' candidates:
// compiled with contraction off, both get the same integers.  The expressions of SURVEY 8(a)-a5, in their order.
struct FacePos { Float3 A, Bv, C; float ax, ay, bx, by, cx, cy; int bx0, by0, bw, bh; unsigned org, ext; };
__device__ inline FacePos face_position(const VertexFwdArgs& a, const float* pa, const float* pb, const float* pc, const float* T) {
    FacePos p;
    p.A = to_camera(pa, T);
    p.Bv = to_camera(pb, T);
    p.C = to_camera(pc, T);
    // perspective_camera: (x*px)/(z*pz), then x multiplier (kaolin rasterises in multiplier units)
    const float apz = p.A.z * a.proj2, bpz = p.Bv.z * a.proj2, cpz = p.C.z * a.proj2;
    p.ax = ((p.A.x * a.proj0) / apz) * a.mult; p.ay = ((p.A.y * a.proj1) / apz) * a.mult;
    p.bx = ((p.Bv.x * a.proj0) / bpz) * a.mult; p.by = ((p.Bv.y * a.proj1) / bpz) * a.mult;
    p.cx = ((p.C.x * a.proj0) / cpz) * a.mult; p.cy = ((p.C.y * a.proj1) / cpz) * a.mult;
    // the pixel box of the face inflated by the soft-mask margin (conservative, see pixel_range), packed for the backward's
    // face sweep: x = px0 | py0 << 16, y = width | height << 16 (0 x 0 if it misses the image)
    face_pixel_box(p.ax, p.ay, p.bx, p.by, p.cx, p.cy, a.infl, a.mult, a.W, a.H, p.bx0, p.by0, p.bw, p.bh, p.org, p.ext);
    return p;
}

// one face: its positions (above), unit normal -> the packed record the pixel stage streams (geo), attributes['face_normals'], cleared face flags
__device__ inline void face_record(const VertexFwdArgs& a, int b, int f, const float* pa, const float* pb, const float* pc, const float* T,
                                   int& bx0, int& by0, int& bw, int& bh) {
    const FacePos p = face_position(a, pa, pb, pc, T);
    const Float3 A = p.A, Bv = p.Bv, C = p.C;
    const float e0[3] = {Bv.x - A.x, Bv.y - A.y, Bv.z - A.z};
    const float e1[3] = {C.x - A.x, C.y - A.y, C.z - A.z};
    float n[3];
    cross3(e0, e1, n);
    const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const float den = len + 1e-10f;
    const float nx = n[0] / den, ny = n[1] / den, nz = n[2] / den;
    const size_t o = (size_t)b * a.F + f;
    a.geo[o * 3 + 0] = make_float4(p.ax, p.ay, p.bx, p.by);
    a.geo[o * 3 + 1] = make_float4(p.cx, p.cy, A.z, Bv.z);
    a.geo[o * 3 + 2] = make_float4(C.z, nz, __uint_as_float(p.org), __uint_as_float(p.ext));
    a.face_normals[o * 3 + 0] = nx; a.face_normals[o * 3 + 1] = ny; a.face_normals[o * 3 + 2] = nz;
    reinterpret_cast<int2*>(a.fflag)[o] = make_int2(0, 0);
    bx0 = p.bx0; by0 = p.by0; bw = p.bw; bh = p.bh;
}

#ifdef MM_VX_ORDER
// ---------------------------------------------------------------------------------------------------------------------
// The ORDER WORKGROUP of image b: the counting sort of the image's tiles by candidate count that order_kernel (mm_raster.hip) does from the
// bin masks -- here from the faces' boxes, which this workgroup forms itself from the step's inputs (face_position: the record path's own
// text), so that it depends on nothing the record workgroups of this launch write.  No hand-off between workgroups, no ticket, no
// write-through store: work repeated on a chip that is nine tenths idle during this launch, in place of a launch and a trip of its own.
//   faces   MM_ORDER_FPT faces per thread and pass: all their corner ids in one trip, all their vertices in the next.  No load stands under a
//           branch: past the mesh's end a lane reads the LAST face again (clamped address) and skips it afterwards.  A load under `if (f < F)`
//           beside a zero for the other lanes was compiled with a wait for memory behind every such load -- a pass's ids came in MM_ORDER_FPT
//           dependent trips, not in one.  (Forming the corners' screen positions once per VERTEX, in LDS, in place of once per corner was
//           built and measured 0.6 us SLOWER: the workgroup is bound by its chain of dependent steps, not by its instruction count;
//           profiles/order_vertex_positions_ab.md)
//   count   a tile's count = the faces whose box touches its bin (8-pixel bins: order_in_vertex, mm_device.h), the bin ranges formed as
//           bin_wave_faces forms them.  A 2-D DIFFERENCE array in LDS: four integer adds per face whatever its box covers (a close-up's faces
//           cover every bin), a row scan and a column scan over the bins (grids of at most 64 x 64 bins: DPP scans, 16, 32 or 64 lanes per
//           line; longer lines: a thread per line).  Integers throughout: the counts are the masks' popcounts exactly
//   sort    as order_kernel: min(count, 1023) per tile slot, histogram, tile_sort_scatter<256, 1>, the same order / nheavy arrays
// ---------------------------------------------------------------------------------------------------------------------
#ifndef MM_ORDER_FPT
#define MM_ORDER_FPT 4        // (8 = every load of a 1 280-face mesh in front of all arithmetic: 166 VGPRs instead of 120, not faster; profiles/order_beside_vertex_ab.md)
#endif
// Inclusive scans of `lines` lines of n <= SEG elements each (element e of line l: s[l * line_stride + e * elem_stride]), in place, by 256
// threads: SEG consecutive lanes take a line, 256 / SEG lines per step.  wave_prefix_excl's DPP steps, stopped where the segment ends: row_shr
// inside the 16-lane rows, row_bcast:15 for segments of 32 and row_bcast:31 for the whole wave.  (The loop's bound is workgroup-uniform:
// every lane is active at the cross-lane steps; lanes past a line's end carry zeros.)  Integer adds: the same sums as a serial scan.
template <int SEG>
__device__ inline void order_scan_lines(int* s, int lines, int n, int line_stride, int elem_stride) {
    static_assert(SEG == 16 || SEG == 32 || SEG == 64, "whole DPP rows");
    const int e = (int)threadIdx.x & (SEG - 1);
    for (int l0 = 0; l0 < lines; l0 += 256 / SEG) {
        const int l = l0 + (int)threadIdx.x / SEG;
        const bool ok = l < lines && e < n;
        int inc = ok ? s[l * line_stride + e * elem_stride] : 0;
        inc += dpp_i32<0x111, 0xF, true>(inc);                   // row_shr:1
        inc += dpp_i32<0x112, 0xF, true>(inc);                   // row_shr:2
        inc += dpp_i32<0x114, 0xF, true>(inc);                   // row_shr:4
        inc += dpp_i32<0x118, 0xF, true>(inc);                   // row_shr:8
        if constexpr (SEG >= 32) inc += dpp_i32<0x142, 0xA, false>(inc);   // row_bcast:15 -> rows 1, 3
        if constexpr (SEG == 64) inc += dpp_i32<0x143, 0xC, false>(inc);   // row_bcast:31 -> rows 2, 3
        if (ok) s[l * line_stride + e * elem_stride] = inc;
    }
}

__device__ inline void order_workgroup(const VertexFwdArgs& a, int b, float* s_trig, Camera* s_cam) {
    __shared__ unsigned short s_key[1024];
    __shared__ int s_start[1024];          // histogram, then the first output position of every key
    __shared__ int s_cnt[1024];            // (nby,nbx) difference array, then the bins' counts; nbx * nby <= tile slots <= 1024
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, nbx = a.nbx, nby = a.nby, nslot = 4 * a.blocks_per_image;
    for (int i = tid; i < 1024; i += 256) { s_start[i] = 0; s_cnt[i] = 0; }
    const float* vb = a.vertices + (size_t)MM_VX_SAMPLE(b) * a.V * 3;
    bool camera = false;
    float T[12];
    for (int f0 = 0; f0 < a.F; f0 += 256 * MM_ORDER_FPT) {
        int id[MM_ORDER_FPT][3];
        float P[MM_ORDER_FPT][9];
#pragma unroll
        for (int k = 0; k < MM_ORDER_FPT; ++k) {                   // consecutive lanes, consecutive faces; past the end: the last face (skipped below)
            const int f = min(f0 + k * 256 + tid, a.F - 1);
            const PackedI3 i3 = *(const PackedI3*)(a.faces + (size_t)f * 3);
            id[k][0] = i3.x; id[k][1] = i3.y; id[k][2] = i3.z;
        }
#pragma unroll
        for (int k = 0; k < MM_ORDER_FPT; ++k) {                   // (every lane holds a face's ids)
#pragma unroll
            for (int c = 0; c < 3; ++c) { const Packed3 v3 = *(const Packed3*)(vb + (size_t)id[k][c] * 3); P[k][c * 3] = v3.x; P[k][c * 3 + 1] = v3.y; P[k][c * 3 + 2] = v3.z; }
        }
        if (!camera) {                                            // (workgroup-uniform; its barriers also put the zeroed LDS behind them)
            block_camera(a.azim, a.elev, a.dist, a.bias, b, s_trig, s_cam);
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = s_cam->T[i];
            camera = true;
        }
#pragma unroll
        for (int k = 0; k < MM_ORDER_FPT; ++k) {
            if (f0 + k * 256 + tid >= a.F) continue;
            const FacePos p = face_position(a, &P[k][0], &P[k][3], &P[k][6], T);
            if (p.bw <= 0 || p.bh <= 0) continue;                 // the box misses the image: no bin (bin_wave_faces)
            const int c0 = p.bx0 >> 3, c1 = (p.bx0 + p.bw - 1) >> 3, r0 = p.by0 >> 3, r1 = (p.by0 + p.bh - 1) >> 3;   // pixel_range clips to the image: c1 < nbx, r1 < nby
            atomicAdd(&s_cnt[r0 * nbx + c0], 1);
            if (c1 + 1 < nbx) atomicAdd(&s_cnt[r0 * nbx + c1 + 1], -1);   // (the entries of column nbx and row nby would be read by no scan)
            if (r1 + 1 < nby) {
                atomicAdd(&s_cnt[(r1 + 1) * nbx + c0], -1);
                if (c1 + 1 < nbx) atomicAdd(&s_cnt[(r1 + 1) * nbx + c1 + 1], 1);
            }
        }
    }
    __syncthreads();
    const int nbmax = max(nbx, nby);
    if (nbmax <= 64) {                                            // row scan, column scan: s_cnt[r][c] = faces whose box touches bin (r, c)
        if (nbmax <= 16) { order_scan_lines<16>(s_cnt, nby, nbx, nbx, 1); __syncthreads(); order_scan_lines<16>(s_cnt, nbx, nby, 1, nbx); }
        else if (nbmax <= 32) { order_scan_lines<32>(s_cnt, nby, nbx, nbx, 1); __syncthreads(); order_scan_lines<32>(s_cnt, nbx, nby, 1, nbx); }
        else { order_scan_lines<64>(s_cnt, nby, nbx, nbx, 1); __syncthreads(); order_scan_lines<64>(s_cnt, nbx, nby, 1, nbx); }
    } else {                                                      // (a strip of a screen: a thread per row, then a thread per column)
        for (int r = tid; r < nby; r += 256) {
            int run = 0;
#pragma unroll 4
            for (int c = 0; c < nbx; ++c) { run += s_cnt[r * nbx + c]; s_cnt[r * nbx + c] = run; }
        }
        __syncthreads();
        for (int c = tid; c < nbx; c += 256) {
            int run = 0;
#pragma unroll 4
            for (int r = 0; r < nby; ++r) { run += s_cnt[r * nbx + c]; s_cnt[r * nbx + c] = run; }
        }
    }
    __syncthreads();
    for (int slot = tid; slot < nslot; slot += 256) {             // (order_kernel's loop, the count read from LDS)
        const int blk = slot >> 2, q = slot & 3;
        const int tx0 = (blk % a.blocks_x) * MM_BLOCK_PX + (q & 1) * MM_TILE, ty0 = (blk / a.blocks_x) * MM_BLOCK_PX + (q >> 1) * MM_TILE;
        int c = 0;
        if (tx0 < a.W && ty0 < a.H) c = s_cnt[(ty0 >> 3) * nbx + (tx0 >> 3)];
        c = min(c, 1023);
        s_key[slot] = (unsigned short)c;
        atomicAdd(&s_start[c], 1);
    }
    tile_sort_scatter<256, 1>(nslot, s_key, s_start, s_wave, a.order + (size_t)b * nslot, a.nheavy + 4 * b);
}
#endif

// kOrder: the launch carries order workgroups.  A kernel of its own (vertex_fwd_order_kernel, below) and not a branch of vertex_fwd_kernel: the
// order workgroups' registers and LDS (120 VGPRs, 10 KB) would be every shape's, and at 13 776 faces and 512x512, where this launch is 43 MB of
// stores from 864 workgroups, the occupancy they cost made it 2.9 us longer (profiles/order_beside_vertex_ab.md).
template <bool kOrder>
__device__ inline void vertex_fwd_body(const VertexFwdArgs& a) {
    __shared__ float s_trig[4];
    __shared__ Camera s_cam;
    const int tid = threadIdx.x;
    for (int i = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid; i < a.ntcnt; i += gridDim.x * gridDim.y * 256) a.tcnt[i] = 0;
    for (int i = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid; i < a.nltot; i += gridDim.x * gridDim.y * 256) a.ltot[i] = 0;
    int b = blockIdx.y;
#ifdef MM_VX_ORDER
    if (kOrder) {
        // The grid's FIRST rows are the order workgroups, one per image: theirs is the launch's longest chain, so they are dispatched in front of
        // the record workgroups (what workgroups that start late cost a launch: profiles/fused_step_kernel_stats.md).  Workgroup-uniform.
        if ((int)blockIdx.y < a.order_rows) {
            const int img = blockIdx.y * gridDim.x + blockIdx.x;
            if (img < a.B) order_workgroup(a, img, s_trig, &s_cam);
            return;
        }
        b -= a.order_rows;
    }
#endif
    // this lane's face: its corner ids and their raw positions depend on nothing the camera produces -- both trips to memory are in
    // flight while four lanes do the fp64 trigonometry and one builds the look-at
    const int f = blockIdx.x * 256 + tid;
    float pa[3] = {0.f, 0.f, 0.f}, pb[3] = {0.f, 0.f, 0.f}, pc[3] = {0.f, 0.f, 0.f};
    if (f < a.F) {
        const int i0 = a.faces[f * 3 + 0], i1 = a.faces[f * 3 + 1], i2 = a.faces[f * 3 + 2];
        const float* vb = a.vertices + (size_t)MM_VX_SAMPLE(b) * a.V * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) { pa[j] = vb[(size_t)i0 * 3 + j]; pb[j] = vb[(size_t)i1 * 3 + j]; pc[j] = vb[(size_t)i2 * 3 + j]; }
    }
    block_camera(a.azim, a.elev, a.dist, a.bias, b, s_trig, &s_cam);
    if (blockIdx.x == 0 && tid < 12) a.T[b * 12 + tid] = s_cam.T[tid];
    if (blockIdx.x == 0 && tid == 12) a.ticket[b] = 0u;
    if (blockIdx.x == 0 && tid >= 64 && tid < 100) a.cam[b * 48 + tid - 64] = reinterpret_cast<const float*>(&s_cam)[tid - 64];
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = s_cam.T[i];

    int bx0 = 0, by0 = 0, bw = 0, bh = 0;                         // inflated pixel box of this lane's face (none)
    if (f < a.F) face_record(a, b, f, pa, pb, pc, T, bx0, by0, bw, bh);

    // ---- screen binning: this wave's 64 faces are exactly mask word c (bin_wave_faces, mm_device.h) ---------------------------
    const int c = blockIdx.x * 4 + (tid >> 6);
    if (a.mask != nullptr && c < a.words) bin_wave_faces(a.mask, b, a.nbx, a.nby, a.words, a.bin_shift, c, tid & 63, bx0, by0, bw, bh);
}

__global__ __launch_bounds__(256) void MM_VX(vertex_fwd_kernel)(VertexFwdArgs a) { vertex_fwd_body<false>(a); }
#ifdef MM_VX_ORDER
__global__ __launch_bounds__(256) void vertex_fwd_order_kernel(VertexFwdArgs a) { vertex_fwd_body<true>(a); }
#endif

struct VertexBwdArgs {
    int B, V, F;
    float proj0, proj1, proj2;
    const int4* vc_table;   // (V,vc_stride) {face*3 + corner, the face's three vertex ids}, padded with -1
    int vc_stride;
    int views;              // images per sample (read by the *_views kernels only; in what was padding); the gradients stay per image
    const int32_t* faces;   // (F,3) vertex ids (the per-image form walks the faces)
    const float* vertices;
    const float *azim, *elev, *dist, *bias;
    const float* T;         // (B,12) saved by the forward
    const float* cam;       // (B,48) the forward's Camera record
    const int2* chunkmap;   // (B,F) {first sweep item, items} of every face
    const float* part;      // (B,item_cap,12) the items' partial sums: dL/d(face xy) (6), dL/d(unit normal) (3)
    int item_cap;
    const float* gfn;       // (B,F,3) external gradient of attributes['face_normals'] or NULL
    float* dTpart;          // (B,groups,12) per-workgroup partial sums of dL/dT
    unsigned* ticket;       // (B) zeroed arrival counter
    int* tcnt; int ntcnt;   // texture-record counters, consumed by the gather before this kernel: cleared for the next backward
    const float* dl_part;   // (B,blocks,12) partial dL/dlights of the pixel backward
    int dl_tiles;           // step mode: dl_part holds one row per TILE, (B,4*blocks,12); a block's row is ((t0 + t1) + t2) + t3, pixel_bwd's own order
    int geometry_only;      // nothing was rasterised (MMRenderDesc.geometry_only): no face has sweep items, no light gradient is written
    int blocks_per_image;
    float* grad_lights;
    float* grad_vertices;
    float *grad_azim, *grad_elev, *grad_dist, *grad_bias;
#ifdef MM_VERTEX_INDEXED
    const int* vrow;        // (B) the row of `vertices` every image reads; the gradients stay per image
#endif
};

#ifndef MM_VBWD_ROWS
#define MM_VBWD_ROWS 4      // item rows per corner and trip (2: -2.5 us at 256x256, -1.5 at 512x512 where faces have several items; equal at 128x128: r06_batch_walk_flags_ab.md)
#endif
// Eight lanes per vertex, grid (ceil(V/32), B).  Per-vertex gradients are gathered through the static vertex->corner
// CSR (no atomics); dT is reduced per workgroup and added to the image's accumulator; the LAST
// workgroup of an image to arrive (agent-scope release / ticket / acquire, cdna_hip_programming.md G16) runs the
// camera chain.
__global__ __launch_bounds__(256) void MM_VX(vertex_bwd_kernel)(VertexBwdArgs a) {
    __shared__ Camera s_cam;
    __shared__ float s_red[4][12];
    __shared__ float s_part[21][12];
    __shared__ int s_last;
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid; i < a.ntcnt; i += gridDim.x * gridDim.y * 256) a.tcnt[i] = 0;
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = a.T[b * 12 + i];
    const float* vb = a.vertices + (size_t)MM_VX_SAMPLE(b) * a.V * 3;
    float acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.f;

    // 8 lanes per vertex: lane c of the group takes corners c, c+8, ... of the vertex (valence is ~6), then a 3-step
    // butterfly inside the group; 32 vertices per workgroup
    const int v = blockIdx.x * 32 + (tid >> 3), cl = tid & 7;
    if (v < a.V) {
        const float p[3] = {vb[v * 3], vb[v * 3 + 1], vb[v * 3 + 2]};
        const Float3 me = to_camera(p, T);
        const float pz = me.z * a.proj2;
        const float ipz = 1.f / pz;                               // one division per vertex, not three per corner
        const float xi = (me.x * a.proj0) * ipz, yi = (me.y * a.proj1) * ipz;
        float d[3] = {0.f, 0.f, 0.f};
        // The vertex's corners from the fixed-stride table: its address depends on nothing but the vertex, so it travels with T and the
        // vertex itself, and the entry carries the face's three vertex ids -- the CSR (offsets -> items -> faces) was two trips more.
        for (int sl8 = cl; sl8 < a.vc_stride; sl8 += 8) {
            const int4 ent = a.vc_table[(size_t)v * a.vc_stride + sl8];
            if (ent.x < 0) break;                                 // padding: this vertex has no further corner
            const int item = ent.x;
            const int f = item / 3, k = item - f * 3;
            const size_t o = (size_t)b * a.F + f;
            // the face's gradients = its sweep items' partial sums, added in index order (one item for most faces)
            float gx = 0.f, gy = 0.f, g[3] = {0.f, 0.f, 0.f};
            const int2 cm = a.geometry_only ? make_int2(0, 0) : a.chunkmap[o];
            // the face's three vertices ride along with chunkmap: loaded whether or not the normal gradient below turns out to be zero
            // -- inside that branch they would cost a dependent trip to memory of their own
            const int i0 = ent.y, i1 = ent.z, i2 = ent.w;
            float pa[3], pb[3], pc[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) { pa[j] = vb[(size_t)i0 * 3 + j]; pb[j] = vb[(size_t)i1 * 3 + j]; pc[j] = vb[(size_t)i2 * 3 + j]; }
            const float* part = a.part + ((size_t)b * a.item_cap + cm.x) * 12;
            // the first MM_VBWD_ROWS items' sums in ONE trip (clamped addresses, selected afterwards: a loop over a per-lane count costs a dependent
            // trip per item); the rest MM_VBWD_ROWS at a time.  Added in index order either way.  (A face has ONE item at 128x128 and the spare rows are
            // re-reads of it that hit the L1: two rows instead of four were measured equal there and slower where faces have several items.)
            float pk[MM_VBWD_ROWS][5];
#pragma unroll
            for (int c = 0; c < MM_VBWD_ROWS; ++c) {
                const float* pc4 = a.part + ((size_t)b * a.item_cap + min(cm.x + min(c, max(cm.y - 1, 0)), a.item_cap - 1)) * 12;   // (a face without items still addresses a valid row)
                pk[c][0] = pc4[k * 2]; pk[c][1] = pc4[k * 2 + 1]; pk[c][2] = pc4[6]; pk[c][3] = pc4[7]; pk[c][4] = pc4[8];
            }
#pragma unroll
            for (int c = 0; c < MM_VBWD_ROWS; ++c) {
                if (c < cm.y) { gx += pk[c][0]; gy += pk[c][1]; g[0] += pk[c][2]; g[1] += pk[c][3]; g[2] += pk[c][4]; }
            }
            for (int c0 = MM_VBWD_ROWS; c0 < cm.y; c0 += MM_VBWD_ROWS) {   // (big faces -- a close-up, a crumpled fine mesh)
#pragma unroll
                for (int c = 0; c < MM_VBWD_ROWS; ++c) {
                    const float* pc4 = part + (size_t)min(c0 + c, cm.y - 1) * 12;
                    pk[c][0] = pc4[k * 2]; pk[c][1] = pc4[k * 2 + 1]; pk[c][2] = pc4[6]; pk[c][3] = pc4[7]; pk[c][4] = pc4[8];
                }
#pragma unroll
                for (int c = 0; c < MM_VBWD_ROWS; ++c) {
                    if (c0 + c < cm.y) { gx += pk[c][0]; gy += pk[c][1]; g[0] += pk[c][2]; g[1] += pk[c][3]; g[2] += pk[c][4]; }
                }
            }
            // through face_vertices_image
            d[0] += gx * a.proj0 * ipz;
            d[1] += gy * a.proj1 * ipz;
            d[2] += -(gx * xi + gy * yi) * a.proj2 * ipz;
            // through the unit face normal
            if (a.gfn) { g[0] += a.gfn[o * 3]; g[1] += a.gfn[o * 3 + 1]; g[2] += a.gfn[o * 3 + 2]; }
            if (g[0] != 0.f || g[1] != 0.f || g[2] != 0.f) {
                const Float3 A = to_camera(pa, T), Bv = to_camera(pb, T), C = to_camera(pc, T);
                const float e0[3] = {Bv.x - A.x, Bv.y - A.y, Bv.z - A.z};
                const float e1[3] = {C.x - A.x, C.y - A.y, C.z - A.z};
                float n[3];
                cross3(e0, e1, n);
                const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
                const float den = len + 1e-10f;
                const float ng = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2];
                // d/dn of g . n / (|n| + 1e-10):  g / den - (n . g) / den^2 * n / |n|   (two divisions for the three components)
                const float iden = 1.f / den, c = (len > 0.f) ? (ng * iden * iden) / len : 0.f;
                float dn[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) dn[j] = g[j] * iden - c * n[j];
                float de0[3], de1[3];
                cross3(e1, dn, de0);
                cross3(dn, e0, de1);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (k == 0) d[j] -= de0[j] + de1[j];
                    else if (k == 1) d[j] += de0[j];
                    else d[j] += de1[j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            d[j] += xchg_f32<4>(d[j], tid); d[j] += xchg_f32<2>(d[j], tid); d[j] += xchg_f32<1>(d[j], tid);
        }
        if (cl == 0) {
            float* gv = a.grad_vertices + ((size_t)b * a.V + v) * 3;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                gv[i] = (T[i * 3 + 0] * d[0] + T[i * 3 + 1] * d[1]) + T[i * 3 + 2] * d[2];
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[i * 3 + j] = p[i] * d[j];
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[9 + j] = d[j];
        }
    }
    const float dT_wg = block_sum_wide(acc, s_red);
    if (tid < 12) {
        // This workgroup's partial of dL/dT, WRITE-THROUGH (agent-scope relaxed atomic store = sc1: it lands at the memory side, not in
        // this XCD's L2), so that the image's last workgroup can read it with agent-scope loads and NO fence on either side
        // (cdna_hip_programming.md G16, form "sc1 stores and sc1 loads on both sides").  No float atomics: the sum below runs
        // over the workgroups in index order, so the camera gradients are bitwise reproducible.
        __hip_atomic_store(a.dTpart + ((size_t)b * gridDim.x + blockIdx.x) * 12 + tid, dT_wg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (blockIdx.x == 0 && !a.geometry_only) {   // dL/dlights (needs nothing of this kernel: the image's FIRST workgroup adds it up, off the last one's tail): sum of the pixel-backward workgroup partials; waves 1..3 take 3 components each, lanes stride over
        // the partials (independent loads), fixed butterfly order
        const int wv = tid >> 6, ln = tid & 63;
        if (wv >= 1) {
            float sum[3] = {0.f, 0.f, 0.f};                      // the three components' loads of four rows in flight together
            for (int k0 = ln; k0 < a.blocks_per_image; k0 += 256) {
                float r[4][3];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + 64 * u;
                    const float* row = a.dl_part + ((size_t)b * a.blocks_per_image + min(k, a.blocks_per_image - 1)) * (a.dl_tiles ? 48 : 12) + (wv - 1) * 3;
                    const bool ok = k < a.blocks_per_image;
                    if (a.dl_tiles) {
#pragma unroll
                        for (int i = 0; i < 3; ++i) r[u][i] = ok ? ((row[i] + row[12 + i]) + row[24 + i]) + row[36 + i] : 0.f;
                    } else { r[u][0] = ok ? row[0] : 0.f; r[u][1] = ok ? row[1] : 0.f; r[u][2] = ok ? row[2] : 0.f; }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) { sum[0] += r[u][0]; sum[1] += r[u][1]; sum[2] += r[u][2]; }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                sum[i] = wave_sum(sum[i]);
                if (ln == 0) a.grad_lights[b * 9 + (wv - 1) * 3 + i] = sum[i];
            }
        }
    }
    // ---- publish, take a ticket; the last workgroup of this image finishes the camera chain (the hand-off: mm_device.h).  The image's ticket
    // is not reset here: thread 0 clears it below, after the camera chain, and the forward clears it too
    if (!last_workgroup(a.ticket + b, gridDim.x, false, s_last)) return;
    if (tid >= 64 && tid < 100) reinterpret_cast<float*>(&s_cam)[tid - 64] = a.cam[b * 48 + tid - 64];   // the forward's camera (no trig here)
    {   // dL/dT = sum of the workgroups' partials in a FIXED order: thread (gl, comp) adds rows gl, gl + 21, gl + 42, ... of its component --
        // all of its loads in flight together: ONE trip to memory however many workgroups the image has (6 890 vertices: 216 rows; a pass of
        // 21 rows at a time was eleven dependent trips, ~20 us of serial tail per image) -- then twelve threads add the 21 partial sums in
        // index order.  No float atomics, the same order every run: bitwise reproducible.
        const int gl = tid / 12, comp = tid - gl * 12;
        float sum = 0.f;
        if (gl < 21) {
            for (unsigned g0 = gl; g0 < gridDim.x; g0 += 21 * 8) {
                float r[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const unsigned g = g0 + 21u * u;
                    r[u] = g < gridDim.x ? __hip_atomic_load(a.dTpart + ((size_t)b * gridDim.x + g) * 12 + comp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) sum += r[u];
            }
            s_part[gl][comp] = sum;
        }
        __syncthreads();
        if (tid < 12) {
            float tot = 0.f;
            for (int k = 0; k < 21; ++k) tot += s_part[k][tid];
            s_red[0][tid] = tot;
        }
    }
    __syncthreads();
    if (tid == 0) {
        float dT[12];
        for (int i = 0; i < 12; ++i) dT[i] = s_red[0][i];
        float dd, de, da, db[2];
        camera_backward(a.dist[b], s_cam, dT, &dd, &de, &da, db);
        a.grad_dist[b] = dd; a.grad_elev[b] = de; a.grad_azim[b] = da;
        a.grad_bias[2 * b] = db[0]; a.grad_bias[2 * b + 1] = db[1];
        a.ticket[b] = 0u;                                        // every workgroup of the image has drawn: ready for the next backward on this workspace
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The vertex backward PER IMAGE, for small templates (at most MM_VIMG_BWD_MAX_FACES faces): ONE workgroup of 1024 threads per image, two
// phases through LDS instead of the ticket / partial-row round trip of vertex_bwd_kernel:
//   A. face-major   a thread per face adds up the face's sweep-item sums (one item for most faces: the first two rows travel with the face's
//                   vertices) and turns them ONCE per face -- not once per corner -- into dL/d(camera-space position) of its three corners:
//                   the screen-space part through the perspective divide, the normal part through the cross product.  Nine floats per face
//                   into LDS.
//   B. vertex-major a thread per vertex adds its corners up in the static table's (ascending) order, writes dL/dvertex and its twelve terms
//                   of dL/dT; one fixed-order workgroup reduction; thread 0 runs the camera chain from the forward's saved record.
// No atomics, no ticket, no write-through partials, no second trip for the image's last workgroup: the chain is {ids, chunk map} ->
// {vertices, item sums} -> LDS -> outputs.  Bitwise reproducible (fixed orders throughout).
// ---------------------------------------------------------------------------------------------------------------------
// (MM_VIMG_BWD_MAX_FACES = 1700, mm_device.h)   36 bytes of LDS per face: 61 KB of dynamic LDS at most, below the 64 KB a launch gets without opting in
__global__ __launch_bounds__(1024) void MM_VX(vertex_image_bwd_kernel)(VertexBwdArgs a) {
    extern __shared__ float s_d[];                                // (F, 3 corners, 3)
    __shared__ Camera s_cam;
    __shared__ float s_red[16][12];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int i = b * 1024 + tid; i < a.ntcnt; i += gridDim.x * 1024) a.tcnt[i] = 0;
    const float* vb = a.vertices + (size_t)MM_VX_SAMPLE(b) * a.V * 3;
    // ---- trip 1: what depends on nothing (T, the camera record, this thread's faces' ids and chunk maps, its vertex and its corner list)
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = a.T[b * 12 + i];
    if (tid >= 64 && tid < 100) reinterpret_cast<float*>(&s_cam)[tid - 64] = a.cam[b * 48 + tid - 64];
    int fid[2][3]; int2 cm[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int f = tid + 1024 * k;
        fid[k][0] = fid[k][1] = fid[k][2] = 0; cm[k] = make_int2(0, 0);
        if (f < a.F) {
            const PackedI3 i3 = *(const PackedI3*)(a.faces + f * 3);
            fid[k][0] = i3.x; fid[k][1] = i3.y; fid[k][2] = i3.z;
            if (!a.geometry_only) cm[k] = a.chunkmap[(size_t)b * a.F + f];
        }
    }
    int it0[8]; float p0[3] = {0.f, 0.f, 0.f};                    // phase B's first vertex: its corner list and position ride along with trip 1
#pragma unroll
    for (int u = 0; u < 8; ++u) it0[u] = (tid < a.V && u < a.vc_stride) ? a.vc_table[(size_t)tid * a.vc_stride + u].x : -1;
    if (tid < a.V) { const Packed3 v3 = *(const Packed3*)(vb + tid * 3); p0[0] = v3.x; p0[1] = v3.y; p0[2] = v3.z; }
    // ---- phase A
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int f = tid + 1024 * k;
        if (f >= a.F) continue;
        const size_t o = (size_t)b * a.F + f;
        float P[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { const Packed3 v3 = *(const Packed3*)(vb + (size_t)fid[k][c] * 3); P[c][0] = v3.x; P[c][1] = v3.y; P[c][2] = v3.z; }
        // the face's gradients = its sweep items' partial sums, added in index order: the first two rows in this trip (clamped addresses,
        // selected afterwards; rows are 48 bytes, 16-byte aligned: three wide loads each), the rare rest one by one
        float r[2][9];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float4* row = (const float4*)(a.part + ((size_t)b * a.item_cap + min(cm[k].x + min(c, max(cm[k].y - 1, 0)), a.item_cap - 1)) * 12);
            const float4 r0 = row[0], r1 = row[1]; const float r2 = a.part[((size_t)b * a.item_cap + min(cm[k].x + min(c, max(cm[k].y - 1, 0)), a.item_cap - 1)) * 12 + 8];
            r[c][0] = r0.x; r[c][1] = r0.y; r[c][2] = r0.z; r[c][3] = r0.w; r[c][4] = r1.x; r[c][5] = r1.y; r[c][6] = r1.z; r[c][7] = r1.w; r[c][8] = r2;
        }
        float gn[3] = {0.f, 0.f, 0.f};
        if (a.gfn) { const Packed3 g3 = *(const Packed3*)(a.gfn + o * 3); gn[0] = g3.x; gn[1] = g3.y; gn[2] = g3.z; }
        float s[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (c < cm[k].y) {
#pragma unroll
                for (int j = 0; j < 9; ++j) s[j] += r[c][j];
            }
        for (int c = 2; c < cm[k].y; ++c) {                       // (a close-up: faces of many 128-pixel chunks)
            const float* row = a.part + ((size_t)b * a.item_cap + cm[k].x + c) * 12;
#pragma unroll
            for (int j = 0; j < 9; ++j) s[j] += row[j];
        }
        const float g[3] = {s[6] + gn[0], s[7] + gn[1], s[8] + gn[2]};
        Float3 cam3[3];
        float d[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            cam3[c] = to_camera(P[c], T);
            const float pz = cam3[c].z * a.proj2;
            const float ipz = 1.f / pz;
            const float xi = (cam3[c].x * a.proj0) * ipz, yi = (cam3[c].y * a.proj1) * ipz;
            const float gx = s[c * 2], gy = s[c * 2 + 1];
            d[c][0] = gx * a.proj0 * ipz;
            d[c][1] = gy * a.proj1 * ipz;
            d[c][2] = -(gx * xi + gy * yi) * a.proj2 * ipz;
        }
        if (g[0] != 0.f || g[1] != 0.f || g[2] != 0.f) {          // through the unit face normal
            const float e0[3] = {cam3[1].x - cam3[0].x, cam3[1].y - cam3[0].y, cam3[1].z - cam3[0].z};
            const float e1[3] = {cam3[2].x - cam3[0].x, cam3[2].y - cam3[0].y, cam3[2].z - cam3[0].z};
            float n[3];
            cross3(e0, e1, n);
            const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            const float den = len + 1e-10f;
            const float ng = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2];
            const float iden = 1.f / den, cc = (len > 0.f) ? (ng * iden * iden) / len : 0.f;
            float dn[3], de0[3], de1[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) dn[j] = g[j] * iden - cc * n[j];
            cross3(e1, dn, de0);
            cross3(dn, e0, de1);
#pragma unroll
            for (int j = 0; j < 3; ++j) { d[0][j] -= de0[j] + de1[j]; d[1][j] += de0[j]; d[2][j] += de1[j]; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 3; ++j) s_d[(f * 3 + c) * 3 + j] = d[c][j];
    }
    __syncthreads();
    // ---- phase B
    float acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.f;
    for (int v = tid; v < a.V; v += 1024) {
        const bool first = v == tid;
        float p[3] = {p0[0], p0[1], p0[2]};
        if (!first) { p[0] = vb[v * 3]; p[1] = vb[v * 3 + 1]; p[2] = vb[v * 3 + 2]; }
        float d[3] = {0.f, 0.f, 0.f};
        for (int sl0 = 0; sl0 < a.vc_stride; sl0 += 8) {          // eight entries per trip (valence is ~6)
            int it[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) it[u] = it0[u];
            if (!first || sl0 != 0) {
#pragma unroll
                for (int u = 0; u < 8; ++u) it[u] = sl0 + u < a.vc_stride ? a.vc_table[(size_t)v * a.vc_stride + sl0 + u].x : -1;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (it[u] >= 0) { d[0] += s_d[it[u] * 3]; d[1] += s_d[it[u] * 3 + 1]; d[2] += s_d[it[u] * 3 + 2]; }
        }
        float* gv = a.grad_vertices + ((size_t)b * a.V + v) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gv[i] = (T[i * 3 + 0] * d[0] + T[i * 3 + 1] * d[1]) + T[i * 3 + 2] * d[2];
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[i * 3 + j] += p[i] * d[j];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[9 + j] += d[j];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = wave_sum(acc[i]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) s_red[tid >> 6][i] = acc[i];
    }
    // dL/dlights: the pixel backward's per-workgroup partials, added by waves 13..15 (three components each; the last waves hold the fewest
    // faces and vertices), lanes stride over the rows, fixed butterfly order
    {
        const int wv = tid >> 6, ln = tid & 63;
        if (wv >= 13 && !a.geometry_only) {
            float sum[3] = {0.f, 0.f, 0.f};
            for (int k0 = ln; k0 < a.blocks_per_image; k0 += 256) {
                float r4[4][3];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int kk = k0 + 64 * u;
                    const float* row = a.dl_part + ((size_t)b * a.blocks_per_image + min(kk, a.blocks_per_image - 1)) * (a.dl_tiles ? 48 : 12) + (wv - 13) * 3;
                    const bool ok = kk < a.blocks_per_image;
                    if (a.dl_tiles) {
#pragma unroll
                        for (int i = 0; i < 3; ++i) r4[u][i] = ok ? ((row[i] + row[12 + i]) + row[24 + i]) + row[36 + i] : 0.f;
                    } else { r4[u][0] = ok ? row[0] : 0.f; r4[u][1] = ok ? row[1] : 0.f; r4[u][2] = ok ? row[2] : 0.f; }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) { sum[0] += r4[u][0]; sum[1] += r4[u][1]; sum[2] += r4[u][2]; }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                sum[i] = wave_sum(sum[i]);
                if (ln == 0) a.grad_lights[b * 9 + (wv - 13) * 3 + i] = sum[i];
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        float dT[12];
        for (int i = 0; i < 12; ++i) {
            float tot = 0.f;
            for (int w = 0; w < 16; ++w) tot += s_red[w][i];
            dT[i] = tot;
        }
        float dd, de, da, db[2];
        camera_backward(a.dist[b], s_cam, dT, &dd, &de, &da, db);
        a.grad_dist[b] = dd; a.grad_elev[b] = de; a.grad_azim[b] = da;
        a.grad_bias[2 * b] = db[0]; a.grad_bias[2 * b + 1] = db[1];
    }
}

// views: images per sample; > 1 goes to the second compilation's launcher (and is what its kernels divide by)
int launch_vertex_fwd_views(const MMRenderDesc* d, const Workspace& w, hipStream_t s, int views);
int launch_vertex_bwd_views(const MMRenderDesc* d, const MMRenderGrads* g, const Workspace& w, hipStream_t s, int views);

int MM_VX(launch_vertex_fwd)(const MMRenderDesc* d, const Workspace& w, hipStream_t s, MM_VX_PARAM) {
#if !defined(MM_VERTEX_VIEWS) && !defined(MM_VERTEX_INDEXED)
    if (views > 1) return launch_vertex_fwd_views(d, w, s, views);
#endif
    VertexFwdArgs a;
    MM_VX_SET(a);
    a.B = d->B; a.V = d->V; a.F = d->F; a.H = d->H; a.W = d->W;
    a.proj0 = d->proj[0]; a.proj1 = d->proj[1]; a.proj2 = d->proj[2]; a.mult = d->multiplier; a.infl = d->boxlen * d->multiplier;
    a.faces = d->faces; a.vertices = d->vertices;
    a.azim = d->azimuths; a.elev = d->elevations; a.dist = d->distances; a.bias = d->biases;
    a.T = w.T; a.cam = w.cam; a.geo = w.geo; a.face_normals = d->face_normals;
    a.tcnt = w.tcnt; a.ntcnt = w.ntcnt + d->B + d->B * w.ntiles;   // (+ the status words and the forward's per-tile counts: cleared by the forward only)
    a.ltot = w.ltot; a.nltot = d->B * MM_LSUB * 4;
    a.bin_shift = w.bin_shift; a.nbx = w.nbx; a.nby = w.nby; a.words = w.words;
    a.mask = d->geometry_only ? nullptr : w.binmask; a.fflag = w.fflag;      // (geometry only: nothing walks the screen bins)
    a.ticket = w.ticket;
    dim3 grid((d->F + 255) / 256, d->B);
#ifdef MM_VX_ORDER
    // the tile sort inside this launch (order workgroups, above) where launch_order would let order_kernel count the mask bits itself; it then
    // launches nothing (one predicate: order_in_vertex, mm_device.h).  This compilation is mm_render_forward's, one view and no index table
    a.order = w.order; a.nheavy = w.nheavy; a.order_rows = 0;
    a.blocks_x = (d->W + MM_BLOCK_PX - 1) / MM_BLOCK_PX; a.blocks_per_image = w.blocks_per_image;
    if (!d->geometry_only && order_in_vertex(d->options, w.blocks_per_image, w.words, w.bin_shift)) {
        a.order_rows = (d->B + (int)grid.x - 1) / (int)grid.x;
        grid.y += (unsigned)a.order_rows;
        ProfScope ps(d->prof_events, MM_PROF_VERTEX_FWD, s);
        hipLaunchKernelGGL(vertex_fwd_order_kernel, grid, dim3(256), 0, s, a);
        return launch_ok("vertex_fwd");
    }
#endif
    { ProfScope ps(d->prof_events, MM_PROF_VERTEX_FWD, s);
      hipLaunchKernelGGL(MM_VX(vertex_fwd_kernel), grid, dim3(256), 0, s, a); }
    return launch_ok("vertex_fwd");
}

int MM_VX(launch_vertex_bwd)(const MMRenderDesc* d, const MMRenderGrads* g, const Workspace& w, hipStream_t s, MM_VX_PARAM) {
#if !defined(MM_VERTEX_VIEWS) && !defined(MM_VERTEX_INDEXED)
    if (views > 1) return launch_vertex_bwd_views(d, g, w, s, views);
#endif
    VertexBwdArgs a;
    MM_VX_SET(a);
    a.B = d->B; a.V = d->V; a.F = d->F;
    a.proj0 = d->proj[0]; a.proj1 = d->proj[1]; a.proj2 = d->proj[2];
    a.vc_table = (const int4*)d->vc_table; a.vc_stride = d->vc_stride; a.vertices = d->vertices;
    a.azim = d->azimuths; a.elev = d->elevations; a.dist = d->distances; a.bias = d->biases;
    a.T = w.T; a.cam = w.cam; a.chunkmap = w.chunkmap; a.part = w.part; a.item_cap = w.item_cap; a.gfn = g->grad_face_normals;
    a.dTpart = w.dTpart; a.ticket = w.ticket;
    a.tcnt = w.tcnt; a.ntcnt = w.ntcnt;
    a.dl_part = w.dl_part; a.dl_tiles = 0; a.blocks_per_image = w.blocks_per_image; a.grad_lights = g->grad_lights;
    if (MM_VX_ONE_VIEW && !d->geometry_only && render_step_mode(d, w)) {
        // step mode: the light rows are the forward's, per tile; and what the forward left in the counters (the images' maxima, cursors and drop
        // counts) is READ by the backward, not consumed -- a second backward after the same forward finds it; the next forward clears it
        a.dl_part = w.dl_tile; a.dl_tiles = 1; a.ntcnt = 0;
    }
    a.grad_vertices = g->grad_vertices;
    a.grad_azim = g->grad_azimuths; a.grad_elev = g->grad_elevations; a.grad_dist = g->grad_distances; a.grad_bias = g->grad_biases;
    a.faces = d->faces; a.geometry_only = d->geometry_only;
    if (vertex_bwd_per_image(d->B, d->F, d->vc_stride)) {
        ProfScope ps(d->prof_events, MM_PROF_VERTEX_BWD, s);
        hipLaunchKernelGGL(MM_VX(vertex_image_bwd_kernel), dim3(d->B), dim3(1024), (size_t)d->F * 9 * sizeof(float), s, a);
        return launch_ok("vertex_image_bwd");
    }
    { ProfScope ps(d->prof_events, MM_PROF_VERTEX_BWD, s);
      hipLaunchKernelGGL(MM_VX(vertex_bwd_kernel), dim3((d->V + 31) / 32, d->B), dim3(256), 0, s, a); }
    return launch_ok("vertex_bwd");
}

}  // namespace mm
