// mm_abi.hip -- extern "C" entry points of libmm_render.so (declared in include/mm_render.h): argument validation,
// workspace carving and launch sequencing.  No allocation, no host synchronisation, no global state.
#include <vector>
#include <cstdio>
#include <cstdlib>
#include "mm_device.h"

namespace mm {
// views: images per sample of a multi-view call (the per-sample inputs then hold B / views rows); 1 = mm_render_forward / mm_render_backward
int launch_vertex_fwd(const MMRenderDesc*, const Workspace&, hipStream_t, int views = 1);
int launch_vertex_bwd(const MMRenderDesc*, const MMRenderGrads*, const Workspace&, hipStream_t, int views = 1);
// index_table: the plan's table of an indexed call (mm_indexed.hip; views == 1 then), nullptr everywhere else
int launch_raster_fwd(const MMRenderDesc*, const Workspace&, hipStream_t, int views = 1, const int* index_table = nullptr);
int launch_raster_bwd(const MMRenderDesc*, const MMRenderGrads*, const Workspace&, hipStream_t, int views = 1, const int* index_table = nullptr);
int launch_view_sum(int B, int views, const float* const* staging, float* const* out, const int* len, hipStream_t);
int launch_vertex_fwd_indexed(const MMRenderDesc*, const Workspace&, hipStream_t, const int* vrow);
int launch_vertex_bwd_indexed(const MMRenderDesc*, const MMRenderGrads*, const Workspace&, hipStream_t, const int* vrow);
int launch_index_plan(int M, const int32_t* const* index, const int* rows, const IndexPlan&, int32_t* status, hipStream_t);
int launch_index_sum(int M, const int* rows, const float* const* staging, float* const* out, const int* len, const IndexPlan&, const MMRenderGrads*, hipStream_t);
int launch_fused_loss(const MMRenderDesc*, const Workspace&, hipStream_t);
size_t recon_workspace_bytes(const MMReconDesc*);
int launch_recon_fwd(const MMReconDesc*, hipStream_t);
int launch_recon_bwd(const MMReconDesc*, hipStream_t);
const float* recon_totals(const MMReconDesc*);
int launch_nn(int, int, int, const float*, const float*, float*, int32_t*, hipStream_t);
int launch_nn_both(int, int, int, const float*, const float*, float*, int32_t*, float*, int32_t*, hipStream_t);
int launch_chamfer_bwd(int, int, int, const float*, const float*, const int32_t*, const int32_t*, const float*, float*, float*, hipStream_t);
size_t reg_workspace_bytes(const MMMeshRegDesc*);
int launch_reg_fwd(const MMMeshRegDesc*, hipStream_t);
int launch_reg_bwd(const MMMeshRegDesc*, const MMMeshRegGrads*, hipStream_t);
size_t att_workspace_bytes(const MMAttLossDesc*);
int launch_att_fwd(const MMAttLossDesc*, hipStream_t);
int launch_att_bwd(const MMAttLossDesc*, const MMAttLossGrads*, hipStream_t);
int launch_disentangle_inputs(const MMDisentangleInputsDesc*, hipStream_t);
size_t disentangle_workspace_bytes(const MMDisentangleDesc*);
int launch_disentangle_fwd(const MMDisentangleDesc*, hipStream_t);
int launch_disentangle_bwd(const MMDisentangleDesc*, const MMDisentangleGrads*, hipStream_t);
int launch_texflow_fwd(const MMTexFlowDesc*, hipStream_t);
int launch_texflow_bwd(const MMTexFlowDesc*, const MMTexFlowGrads*, hipStream_t);
size_t ssim_workspace_bytes(const MMSsimDesc*);
int launch_ssim_fwd(const MMSsimDesc*, hipStream_t);
int launch_ssim_bwd(const MMSsimDesc*, const MMSsimGrads*, hipStream_t);
size_t encfeat_workspace_bytes(int B, int C, int H, int W, int V, int nparts);
int launch_shape_feat_fwd(const MMShapeFeatDesc*, hipStream_t);
int launch_shape_feat_bwd(const MMShapeFeatDesc*, const MMShapeFeatGrads*, hipStream_t);
int launch_camera_feat_fwd(const MMCameraFeatDesc*, hipStream_t);
int launch_camera_feat_bwd(const MMCameraFeatDesc*, const MMCameraFeatGrads*, hipStream_t);
size_t interp_workspace_bytes(int B);
int launch_mix_fwd(const MMInterpDesc*, hipStream_t);
int launch_mix_bwd(const MMInterpDesc*, const MMInterpGrads*, hipStream_t);
int launch_collapse_resample(int B, int V, const float* dv, int* idx_a, int* idx_b, const float* u, float thr, int* n_bad, hipStream_t);
int critic_chunks_per_image(const MMCriticDesc*);
int launch_critic_fwd(const MMCriticDesc*, hipStream_t);
int launch_critic_bwd(const MMCriticDesc*, const MMCriticGrads*, hipStream_t);
void export_grid_geometry(const MMExportDesc*, long long* xmaps, long long* pad, long long* Hg, long long* Wg);
int launch_export_images(const MMExportDesc*, hipStream_t);
int launch_export_grid(const MMExportDesc*, hipStream_t);
struct BatchArgs;
long long batch_lds_bytes(const MMBatchDesc*, BatchArgs*);
int launch_assemble_batch(const MMBatchDesc*, hipStream_t);
struct CompArgs;
long long composite_lds_bytes(const MMCompositeDesc*, CompArgs*);
int launch_composite(const MMCompositeDesc*, hipStream_t);
struct PyrArgs;
long long pyramid_lds_bytes(const MMPyramidDesc*, PyrArgs*);
int launch_pyramid(const MMPyramidDesc*, hipStream_t);
struct PoiArgs;
long long poisson_lds_bytes(const MMPoissonDesc*, PoiArgs*);
int launch_poisson(const MMPoissonDesc*, hipStream_t);
size_t jpeg_workspace_bytes(const MMJpegModesDesc*);
size_t jpeg_files_at(const MMJpegModesDesc*);
int launch_jpeg(const MMJpegModesDesc*, hipStream_t);
size_t jpeg_coef_at(const MMJpegModesDesc*);
int jpeg_layout_of(int mode, int sampling);
long long jpeg_frame_blocks(int H, int W, int layout);
size_t jpeg_roundtrip_workspace_bytes(const MMJpegRoundtripDesc*);
int launch_jpeg_roundtrip(const MMJpegRoundtripDesc*, hipStream_t);
size_t gif_workspace_bytes(const MMGifDesc*);
size_t gif_file_at(const MMGifDesc*);
int launch_gif(const MMGifDesc*, hipStream_t);
size_t png_workspace_bytes(const MMPngDesc*);
size_t png_files_at(const MMPngDesc*);
long long png_idat_cap(const MMPngDesc*);
long long png_all_segs(const MMPngDesc*);
int launch_png(const MMPngDesc*, hipStream_t);
int check_jpeg_decode(const MMJpegDecodeDesc*);
size_t jpeg_decode_workspace_bytes(const MMJpegDecodeDesc*);
int launch_jpeg_decode(const MMJpegDecodeDesc*, hipStream_t);
int check_png_decode(const MMPngDecodeDesc*);
size_t png_decode_workspace_bytes(const MMPngDecodeDesc*);
int launch_png_decode(const MMPngDecodeDesc*, hipStream_t);
int launch_fid_input(const MMFidInputDesc*, hipStream_t);
size_t fid_stats_workspace_bytes(const MMFidStatsDesc*);
int launch_fid_stats(const MMFidStatsDesc*, hipStream_t);
}  // namespace mm

static bool sizes_positive(const MMRenderDesc* d) { return d->B > 0 && d->H > 0 && d->W > 0 && d->V > 0 && d->F > 0 && d->Ht > 0 && d->Wt > 0; }

// the render workspace of `d` as the kernels see it; placed = false: its layout alone, at address 0 with the minimum's record pool
static mm::Workspace carve(const MMRenderDesc* d, bool placed = true) {
    const bool geo = d->geometry_only != 0, step = d->step_grads != nullptr;
    return mm::carve_workspace(placed ? d->workspace : nullptr, d->B, d->V, d->F, d->H, d->W, d->Ht, d->Wt, placed ? d->workspace_bytes : 0, geo, step);
}

static int check_render(const MMRenderDesc* d, bool backward) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (!sizes_positive(d)) return MM_ERR_BAD_SHAPE;
    if (d->knum <= 0) return MM_ERR_UNSUPPORTED;
    if (d->H > 65535 || d->W > 65535) return MM_ERR_UNSUPPORTED;                 // pixel boxes are packed in 16 + 16 bits
    if (d->geometry_only) {                                                       // vertex stage only: what it reads and writes
        if (!d->faces || !d->vertices || !d->azimuths || !d->elevations || !d->distances || !d->biases || !d->face_normals) return MM_ERR_NULL_POINTER;
    } else {
        if (!d->faces || !d->face_uvs || !d->vertices || !d->textures || !d->lights || !d->azimuths || !d->elevations ||
            !d->distances || !d->biases || !d->face_idx || !d->face_normals)
            return MM_ERR_NULL_POINTER;
        if (!backward && !d->rgba) return MM_ERR_NULL_POINTER;                    // (the backward never reads the image: rgba may be NULL there)
        if (d->no_mask && !d->bg) return MM_ERR_NULL_POINTER;
    }
    if (d->fused_gt && !d->geometry_only) {                                       // the contour term of the fused loss (include/mm_render.h)
        if (!(d->fused_contour >= 0.f)) return MM_ERR_BAD_SHAPE;
        if (d->fused_contour > 0.f && ((d->H & 3) || (d->W & 3))) return MM_ERR_BAD_SHAPE;
    }
    if (d->fused_totals) {                                                        // deferred fusion: the backward of a render whose recon_data ran on its own
        if (!backward || d->geometry_only) return MM_ERR_UNSUPPORTED;
        if (!d->fused_gt) return MM_ERR_NULL_POINTER;
        if (d->fused_contour != 0.f) return MM_ERR_UNSUPPORTED;
    }
    if (backward && !d->vc_table) return MM_ERR_NULL_POINTER;
    if (backward && d->vc_stride <= 0) return MM_ERR_BAD_SHAPE;
    if (!d->workspace || d->workspace_bytes < mm_query_workspace(d) || ((uintptr_t)d->workspace & 255)) return MM_ERR_WORKSPACE;
    return MM_OK;
}

// what mm_composite_frames, mm_pyramid_frames and mm_poisson_frames (MMCompositeDesc, MMPyramidDesc, MMPoissonDesc) refuse alike: pointers, sizes, the rounding, a reflection
// pad that would reflect twice, and the host's copy of the two index tables in front of params
template <class Desc>
static int check_frames(const Desc* d) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (!d->renders || !d->backgrounds || !d->params_host || !d->params || !d->out) return MM_ERR_NULL_POINTER;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->n_fg <= 0 || d->n_bg <= 0 || (d->bg_C != 3 && d->bg_C != 4)) return MM_ERR_BAD_SHAPE;
    if (d->rounding != 0 && d->rounding != 1) return MM_ERR_BAD_SHAPE;
    if (d->H > (1 << 24) || d->W > (1 << 24)) return MM_ERR_BAD_SHAPE;      // sums of sizes and pads stay far inside an int32
    const int32_t* bp = d->bg_pad;                                // a reflection reflects once: the pad is narrower than the image
    if (bp[0] < 0 || bp[1] < 0 || bp[2] < 0 || bp[3] < 0 || bp[0] >= d->W || bp[1] >= d->W || bp[2] >= d->H || bp[3] >= d->H) return MM_ERR_BAD_SHAPE;
    const int32_t* par = d->params_host;
    for (int o = 0; o < d->B; ++o)
        if (par[o] < 0 || par[o] >= d->n_fg || par[d->B + o] < 0 || par[d->B + o] >= d->n_bg) return MM_ERR_BAD_SHAPE;
    return MM_OK;
}

// the n_out resize rows at `row` (both kernels' rows are MM_COMPOSITE_ROW_WORDS: mm_frame.h), of an axis of n_in behind its pad; leaves `row` behind them
static int check_resize_rows(const int32_t*& row, int32_t n_out, int32_t n_in) {
    for (int i = 0; i < n_out; ++i, row += MM_COMPOSITE_ROW_WORDS)
        if (row[1] < 1 || row[1] > MM_COMPOSITE_MAX_TAPS || row[0] < 0 || row[0] > n_in - row[1]) return MM_ERR_BAD_SHAPE;
    return MM_OK;
}

extern "C" {

size_t mm_query_workspace(const MMRenderDesc* d) {
    if (!d || !sizes_positive(d)) return 0;
    return carve(d, false).bytes;
}

int mm_render_forward(const MMRenderDesc* d, mm_stream_t stream) {
    int st = check_render(d, false);
    if (st != MM_OK) return st;
    const mm::Workspace w = carve(d);
    hipStream_t s = (hipStream_t)stream;
    mm::clear_stale_error();
    st = mm::launch_vertex_fwd(d, w, s);
    if (st != MM_OK || d->geometry_only) return st;
    return mm::launch_raster_fwd(d, w, s);      // tile order + raster
}

int mm_render_fused_loss(const MMRenderDesc* d, mm_stream_t stream) {
    int st = check_render(d, false);
    if (st != MM_OK) return st;
    if (!d->fused_gt || !d->fused_loss) return MM_ERR_NULL_POINTER;
    const mm::Workspace w = carve(d);
    mm::clear_stale_error();
    return mm::launch_fused_loss(d, w, (hipStream_t)stream);
}

int mm_debug_workspace_layout(const MMRenderDesc* d, size_t* out5) {
    if (!d || !out5) return MM_ERR_NULL_POINTER;
    const mm::Workspace w = mm::carve_workspace(nullptr, d->B, d->V, d->F, d->H, d->W, d->Ht, d->Wt, 0, false, d->step_grads != nullptr);
    out5[0] = (size_t)((char*)w.chunkmap - (char*)nullptr); out5[1] = (size_t)((char*)w.items - (char*)nullptr);
    out5[2] = (size_t)((char*)w.nitems - (char*)nullptr); out5[3] = (size_t)((char*)w.part - (char*)nullptr); out5[4] = (size_t)w.item_cap;
    out5[5] = (size_t)((char*)w.gp - (char*)nullptr); out5[6] = (size_t)((char*)w.gp2 - (char*)nullptr); out5[7] = (size_t)((char*)w.soft - (char*)nullptr);
    out5[8] = (size_t)((char*)w.tcnt - (char*)nullptr); out5[9] = (size_t)w.ntiles; out5[10] = (size_t)w.trcap; out5[11] = (size_t)((char*)w.trcnt - (char*)nullptr);
    return MM_OK;
}

int mm_render_step_mode(const MMRenderDesc* d) {
    if (!d || !sizes_positive(d)) return 0;
    const mm::Workspace w = carve(d, false);
    return mm::render_step_mode(d, w) ? 1 : 0;
}

int mm_debug_step_layout(const MMRenderDesc* d, size_t* out4) {
    if (!d || !out4) return MM_ERR_NULL_POINTER;
    const mm::Workspace w = mm::carve_workspace(nullptr, d->B, d->V, d->F, d->H, d->W, d->Ht, d->Wt, d->workspace_bytes, d->geometry_only != 0, d->step_grads != nullptr);
    out4[0] = (size_t)((char*)w.nheavy - (char*)nullptr); out4[1] = (size_t)((char*)w.dl_tile - (char*)nullptr);
    out4[2] = (size_t)((char*)w.runs - (char*)nullptr); out4[3] = (size_t)w.runcap;
    return MM_OK;
}

int mm_render_status(const MMRenderDesc* d, mm_stream_t stream, int32_t* dropped_host) {
    if (!d) return MM_ERR_NULL_POINTER;                            // (only the shape and the workspace are looked at)
    if (!sizes_positive(d)) return MM_ERR_BAD_SHAPE;
    if (!d->workspace) return MM_ERR_NULL_POINTER;
    if (d->workspace_bytes < mm_query_workspace(d) || ((uintptr_t)d->workspace & 255)) return MM_ERR_BAD_SHAPE;   // (MM_ERR_WORKSPACE is this call's "records were dropped")
    const mm::Workspace w = carve(d);
    std::vector<int32_t> h((size_t)d->B);
    if (hipMemcpyAsync(h.data(), w.tstatus, (size_t)d->B * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) return MM_ERR_LAUNCH;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return MM_ERR_LAUNCH;
    bool any = false;
    for (int b = 0; b < d->B; ++b) { any = any || h[b] != 0; if (dropped_host) dropped_host[b] = h[b]; }
    return any ? MM_ERR_WORKSPACE : MM_OK;
}

int mm_render_backward(const MMRenderDesc* d, const MMRenderGrads* g, mm_stream_t stream) {
    int st = check_render(d, true);
    if (st != MM_OK) return st;
    if (!g || !g->grad_vertices || !g->grad_azimuths || !g->grad_elevations || !g->grad_distances || !g->grad_biases) return MM_ERR_NULL_POINTER;
    const mm::Workspace w = carve(d);
    hipStream_t s = (hipStream_t)stream;
    if (d->geometry_only) {                                       // nothing was rasterised: the gradient arrives through face_normals alone
        if (!g->grad_face_normals) return MM_ERR_NULL_POINTER;
        mm::clear_stale_error();
        return mm::launch_vertex_bwd(d, g, w, s);
    }
    if ((!g->grad_rgba && !d->fused_gt) || !g->grad_textures || !g->grad_lights) return MM_ERR_NULL_POINTER;
    if (d->no_mask && !g->grad_bg) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    st = mm::launch_raster_bwd(d, g, w, s);
    if (st != MM_OK) return st;
    return mm::launch_vertex_bwd(d, g, w, s);
}

// ---- multi-view and indexed renders (include/mm_render.h: MMRenderViewsDesc, MMRenderIndexedDesc) ------------------------------------------
// Both render the images of a sub-descriptor `r`: the caller's MMRenderDesc with a HEAD stripped off its workspace (the images' render workspace
// follows the head with exactly the bytes that are left, as mm_render_forward would be given them).  Both end their backward with a row sum
// (mm_row_sum.h) of the per-image gradients of vertices, textures, lights and bg, which the kernels write into staging areas in the head,
// (images, row) floats each:
struct ViewsStaging { size_t off[4]; int len[4]; size_t bytes; };
static ViewsStaging views_staging(const MMRenderDesc* d) {
    ViewsStaging st;
    const size_t rows[4] = {(size_t)d->V * 3, (size_t)3 * d->Ht * d->Wt, 9, (size_t)3 * d->H * d->W};
    size_t o = 0;
    for (int t = 0; t < 4; ++t) { st.off[t] = o; st.len[t] = (int)rows[t]; o += mm::align256((size_t)d->B * rows[t] * sizeof(float)); }
    st.bytes = o;
    return st;
}
static bool row_lengths_fit(const MMRenderDesc* d) { return (size_t)3 * d->Ht * d->Wt <= 0x7fffffff && (size_t)3 * d->H * d->W <= 0x7fffffff; }

// What both calls' checks end with, before any launch: the modes not built over views or indices, `own` (the caller's verdict on its own
// fields), then *r = the descriptor of the images as the render kernels take it (the workspace without its `head` bytes).
static int check_sub_render(const MMRenderDesc* d, bool backward, int own, size_t head, MMRenderDesc* r) {
    if (d->fused_gt || d->fused_totals || d->geometry_only) return MM_ERR_UNSUPPORTED;    // fused / deferred losses and geometry-only: not built
    if (own != MM_OK) return own;
    *r = *d; r->step_grads = nullptr;                            // (step mode is a single-view, fused mode: the field is ignored here)
    r->workspace = d->workspace ? (char*)d->workspace + head : nullptr;      // (the head is a multiple of 256: the alignment is the caller's)
    r->workspace_bytes = d->workspace_bytes > head ? d->workspace_bytes - head : 0;
    return check_render(r, backward);
}

// a backward whose per-image gradients are summed: every pointer of the nine (bg under no_mask) is needed
static bool grads_complete(const MMRenderGrads* g, bool no_mask) {
    return g && g->grad_vertices && g->grad_azimuths && g->grad_elevations && g->grad_distances && g->grad_biases && g->grad_rgba && g->grad_textures && g->grad_lights && (!no_mask || g->grad_bg);
}

// The per-image gradients `gi` the backward kernels write -- into the staging areas `st` lays out at `base`, or straight into the caller's
// where base is NULL (one view: nothing to sum) -- and the four outputs `out` a row sum reduces `staging` (rows of st.len floats) to.
struct StagedGrads {
    MMRenderGrads gi;
    ViewsStaging st;
    float *staging[4] = {}, *out[4];
    StagedGrads(const MMRenderGrads* g, const ViewsStaging& st, char* base, bool no_mask) : gi(*g), st(st), out{g->grad_vertices, g->grad_textures, g->grad_lights, no_mask ? g->grad_bg : nullptr} {
        if (!base) return;
        for (int t = 0; t < 4; ++t) staging[t] = (float*)(base + st.off[t]);
        gi.grad_vertices = staging[0]; gi.grad_textures = staging[1]; gi.grad_lights = staging[2]; gi.grad_bg = no_mask ? staging[3] : nullptr;
    }
};

// the head of a multi-view workspace: the staging areas (B*N rows each); one view has none
static int check_render_views(const MMRenderViewsDesc* v, bool backward, MMRenderDesc* r) {
    if (!v) return MM_ERR_NULL_POINTER;
    const MMRenderDesc* d = &v->render;
    if (!sizes_positive(d) || v->views < 1 || d->B % v->views != 0) return MM_ERR_BAD_SHAPE;
    // (the verdict is computed here and handed in: check_sub_render returns it AFTER its modes test, where this refusal has always stood)
    const int own = !row_lengths_fit(d) || d->B / v->views > 65535 ? MM_ERR_UNSUPPORTED : MM_OK;
    return check_sub_render(d, backward, own, v->views > 1 ? views_staging(d).bytes : 0, r);
}

static int check_recon(const MMReconDesc* d, bool backward) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0) return MM_ERR_BAD_SHAPE;
    if (!d->pred || !d->gt) return MM_ERR_NULL_POINTER;
    if (!backward && !d->loss) return MM_ERR_NULL_POINTER;
    if (backward && !d->grad_pred) return MM_ERR_NULL_POINTER;
    if (d->contour > 0.f && (d->H < 4 || d->W < 4)) return MM_ERR_BAD_SHAPE;
    if (!d->workspace || d->workspace_bytes < mm_recon_query_workspace(d)) return MM_ERR_WORKSPACE;
    return MM_OK;
}

size_t mm_render_views_query_workspace(const MMRenderViewsDesc* v) {
    if (!v || v->views < 1 || v->render.B <= 0 || v->render.B % v->views != 0) return 0;
    const size_t base = mm_query_workspace(&v->render);
    return base == 0 || v->views == 1 ? base : base + views_staging(&v->render).bytes;
}

int mm_render_views_forward(const MMRenderViewsDesc* v, mm_stream_t stream) {
    MMRenderDesc r;
    int st = check_render_views(v, false, &r);
    if (st != MM_OK) return st;
    const mm::Workspace w = carve(&r);
    hipStream_t s = (hipStream_t)stream;
    mm::clear_stale_error();
    st = mm::launch_vertex_fwd(&r, w, s, v->views);
    if (st != MM_OK) return st;
    return mm::launch_raster_fwd(&r, w, s, v->views);
}

int mm_render_views_backward(const MMRenderViewsDesc* v, const MMRenderGrads* g, mm_stream_t stream) {
    MMRenderDesc r;
    int st = check_render_views(v, true, &r);
    if (st != MM_OK) return st;
    if (!grads_complete(g, r.no_mask)) return MM_ERR_NULL_POINTER;
    const mm::Workspace w = carve(&r);
    hipStream_t s = (hipStream_t)stream;
    const StagedGrads sg(g, views_staging(&r), v->views > 1 ? (char*)v->render.workspace : nullptr, r.no_mask != 0);
    mm::clear_stale_error();
    st = mm::launch_raster_bwd(&r, &sg.gi, w, s, v->views);
    if (st != MM_OK) return st;
    st = mm::launch_vertex_bwd(&r, &sg.gi, w, s, v->views);
    if (st != MM_OK || v->views == 1) return st;
    return mm::launch_view_sum(r.B / v->views, v->views, sg.staging, sg.out, sg.st.len, s);
}

// The head of an indexed workspace: the plan (mm_indexed.hip) -- the table (5, M), then per tensor offsets (rows + 1), cursors (rows) and
// images (M) -- and, for a call with a backward, the staging areas `st` (M rows each) at `staging`.  rows[]: the row counts the kernels go by
// (bg without no_mask: M rows, the identity, never summed).
struct IndexedHead { size_t table, offsets[4], cursor[4], images[4], staging, bytes; int rows[4]; ViewsStaging st; };
static IndexedHead indexed_head(const MMRenderIndexedDesc* v) {
    IndexedHead h;
    const MMRenderDesc* d = &v->render;
    const size_t M = (size_t)d->B;
    size_t o = 0;
    h.table = o; o += mm::align256(5 * M * sizeof(int));
    for (int t = 0; t < 4; ++t) {
        h.rows[t] = (t == 3 && !d->no_mask) ? d->B : v->rows[t];
        const size_t R = (size_t)(h.rows[t] > 0 ? h.rows[t] : 0);
        h.offsets[t] = o; o += mm::align256((R + 1) * sizeof(int));
        h.cursor[t] = o; o += mm::align256(R * sizeof(int));
        h.images[t] = o; o += mm::align256(M * sizeof(int));
    }
    h.st = views_staging(d); h.staging = o;
    h.bytes = o + (v->backward ? h.st.bytes : 0);
    return h;
}
static mm::IndexPlan indexed_plan(const IndexedHead& h, void* workspace) {
    mm::IndexPlan p;
    char* base = (char*)workspace;
    p.table = (int*)(base + h.table);
    for (int t = 0; t < 4; ++t) { p.offsets[t] = (int*)(base + h.offsets[t]); p.cursor[t] = (int*)(base + h.cursor[t]); p.images[t] = (int*)(base + h.images[t]); }
    return p;
}
// the sizes alone (what the query can refuse): MM_OK, or why not
static int indexed_shape(const MMRenderIndexedDesc* v) {
    if (!v) return MM_ERR_NULL_POINTER;
    const MMRenderDesc* d = &v->render;
    if (!sizes_positive(d)) return MM_ERR_BAD_SHAPE;
    if (d->B > 65535) return MM_ERR_UNSUPPORTED;                  // (rows and images are 16-bit keys of the plan; rows are the sum's grid y)
    for (int t = 0; t < 4; ++t) {
        if (t == 3 && !d->no_mask) continue;                      // (no bg in this call: its row count is not looked at)
        if (v->rows[t] < 1) return MM_ERR_BAD_SHAPE;
        if (v->rows[t] > 65535) return MM_ERR_UNSUPPORTED;
    }
    return row_lengths_fit(d) ? MM_OK : MM_ERR_UNSUPPORTED;
}

static int check_render_indexed(const MMRenderIndexedDesc* v, bool backward, MMRenderDesc* r, IndexedHead* h) {
    const int st = indexed_shape(v);
    if (st != MM_OK) return st;
    const MMRenderDesc* d = &v->render;
    // computed early, returned by check_sub_render after its modes test (the refusal order); BAD_SHAPE is assigned last because it outranks WORKSPACE
    int own = backward && !v->backward ? MM_ERR_WORKSPACE : MM_OK;      // a forward-only call left no staging
    for (int t = 0; t < 4; ++t)
        if (!(t == 3 && !d->no_mask) && !v->index[t] && v->rows[t] != d->B) own = MM_ERR_BAD_SHAPE;   // the identity needs a row per image
    *h = indexed_head(v);
    return check_sub_render(d, backward, own, h->bytes, r);
}

size_t mm_render_indexed_query_workspace(const MMRenderIndexedDesc* v) {
    if (indexed_shape(v) != MM_OK) return 0;
    const size_t base = mm_query_workspace(&v->render);
    return base ? base + indexed_head(v).bytes : 0;
}

int mm_render_indexed_forward(const MMRenderIndexedDesc* v, mm_stream_t stream) {
    MMRenderDesc r; IndexedHead h;
    int st = check_render_indexed(v, false, &r, &h);
    if (st != MM_OK) return st;
    const mm::Workspace w = carve(&r);
    const mm::IndexPlan p = indexed_plan(h, v->render.workspace);
    hipStream_t s = (hipStream_t)stream;
    const int32_t* index[4] = {v->index[0], v->index[1], v->index[2], r.no_mask ? v->index[3] : nullptr};
    mm::clear_stale_error();
    st = mm::launch_index_plan(r.B, index, h.rows, p, v->status_flag, s);
    if (st != MM_OK) return st;
    st = mm::launch_vertex_fwd_indexed(&r, w, s, p.table);       // (the table's first row: the images' vertices)
    if (st != MM_OK) return st;
    return mm::launch_raster_fwd(&r, w, s, 1, p.table);
}

int mm_render_indexed_backward(const MMRenderIndexedDesc* v, const MMRenderGrads* g, mm_stream_t stream) {
    MMRenderDesc r; IndexedHead h;
    int st = check_render_indexed(v, true, &r, &h);
    if (st != MM_OK) return st;
    if (!grads_complete(g, r.no_mask)) return MM_ERR_NULL_POINTER;
    const mm::Workspace w = carve(&r);
    const mm::IndexPlan p = indexed_plan(h, v->render.workspace);
    hipStream_t s = (hipStream_t)stream;
    const StagedGrads sg(g, h.st, (char*)v->render.workspace + h.staging, r.no_mask != 0);
    mm::clear_stale_error();
    st = mm::launch_raster_bwd(&r, &sg.gi, w, s, 1, p.table);
    if (st != MM_OK) return st;
    st = mm::launch_vertex_bwd_indexed(&r, &sg.gi, w, s, p.table);
    if (st != MM_OK) return st;
    return mm::launch_index_sum(r.B, h.rows, sg.staging, sg.out, sg.st.len, p, g, s);
}

size_t mm_recon_query_workspace(const MMReconDesc* d) {
    if (!d || d->B <= 0) return 0;
    return mm::recon_workspace_bytes(d);
}

int mm_recon_data_forward(const MMReconDesc* d, mm_stream_t stream) {
    int st = check_recon(d, false);
    if (st != MM_OK) return st;
    mm::clear_stale_error();
    return mm::launch_recon_fwd(d, (hipStream_t)stream);
}

int mm_recon_data_backward(const MMReconDesc* d, mm_stream_t stream) {
    int st = check_recon(d, true);
    if (st != MM_OK) return st;
    mm::clear_stale_error();
    return mm::launch_recon_bwd(d, (hipStream_t)stream);
}

const float* mm_recon_data_totals(const MMReconDesc* d) {
    if (!d || d->B <= 0 || !d->workspace || d->workspace_bytes < mm_recon_query_workspace(d)) return nullptr;
    return mm::recon_totals(d);
}

int mm_nearest_neighbour(int32_t B, int32_t N, int32_t M, const float* x, const float* y, float* dist, int32_t* idx,
                         mm_stream_t stream) {
    if (!x || !y || !dist || !idx) return MM_ERR_NULL_POINTER;
    if (B <= 0 || N <= 0 || M <= 0) return MM_ERR_BAD_SHAPE;
    if (B > 65535) return MM_ERR_UNSUPPORTED;                     // (batch rows are the grid's y dimension)
    mm::clear_stale_error();
    return mm::launch_nn(B, N, M, x, y, dist, idx, (hipStream_t)stream);
}

int mm_chamfer_nearest(int32_t B, int32_t N, int32_t M, const float* x, const float* y, float* dist_x, int32_t* idx_x,
                       float* dist_y, int32_t* idx_y, mm_stream_t stream) {
    if (!x || !y || !dist_x || !idx_x || !dist_y || !idx_y) return MM_ERR_NULL_POINTER;
    if (B <= 0 || N <= 0 || M <= 0) return MM_ERR_BAD_SHAPE;
    if (B > 65535) return MM_ERR_UNSUPPORTED;
    mm::clear_stale_error();
    return mm::launch_nn_both(B, N, M, x, y, dist_x, idx_x, dist_y, idx_y, (hipStream_t)stream);
}

int mm_chamfer_backward(int32_t B, int32_t N, int32_t M, const float* x, const float* y, const int32_t* idx_x, const int32_t* idx_y,
                        const float* grad_loss, float* grad_x, float* grad_y, mm_stream_t stream) {
    if (!x || !y || !idx_x || !idx_y || !grad_loss || !grad_x || !grad_y) return MM_ERR_NULL_POINTER;
    if (B <= 0 || N <= 0 || M <= 0) return MM_ERR_BAD_SHAPE;
    if (B > 65535) return MM_ERR_UNSUPPORTED;
    mm::clear_stale_error();
    return mm::launch_chamfer_bwd(B, N, M, x, y, idx_x, idx_y, grad_loss, grad_x, grad_y, (hipStream_t)stream);
}

static int check_reg(const MMMeshRegDesc* d, bool backward) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->B <= 0 || d->V <= 0 || d->F <= 0 || d->E < 0) return MM_ERR_BAD_SHAPE;
    if (d->terms == 0 || d->terms >= (1u << MM_REG_TERMS)) return MM_ERR_BAD_SHAPE;
    const unsigned need_v = (1u << MM_REG_EDGE) | (1u << MM_REG_DEPTH) | (1u << MM_REG_DEPTHR) | (1u << MM_REG_DEPTHC);
    const unsigned need_d = (1u << MM_REG_LAPLACIAN) | (1u << MM_REG_DEFORM) | (1u << MM_REG_FLIP);
    if ((d->terms & need_v) && (!d->vertices || !d->sign_init)) return MM_ERR_NULL_POINTER;
    if ((d->terms & need_d) && !d->delta_vertices) return MM_ERR_NULL_POINTER;
    if ((d->terms & (1u << MM_REG_FLAT)) && (!d->face_normals || !d->edge2faces || (backward && (!d->fe_offsets || !d->fe_items)))) return MM_ERR_NULL_POINTER;
    if ((d->terms & (1u << MM_REG_LAPLACIAN)) && (!d->lap_offsets || !d->lap_cols || !d->lap_vals ||
                                                   (backward && (!d->lapT_offsets || !d->lapT_cols || !d->lapT_vals)))) return MM_ERR_NULL_POINTER;
    if ((d->terms & (1u << MM_REG_EDGE)) && (!d->edges || (backward && (!d->ve_offsets || !d->ve_items)))) return MM_ERR_NULL_POINTER;
    if ((d->terms & (1u << MM_REG_FLIP)) && (!d->flip_index || !d->sign_init || (backward && (!d->flipT_offsets || !d->flipT_items)))) return MM_ERR_NULL_POINTER;
    if ((d->terms & ((1u << MM_REG_DEPTHR) | (1u << MM_REG_DEPTHC))) && !(d->ratio > 0.f)) return MM_ERR_BAD_SHAPE;
    if (!backward && !d->losses) return MM_ERR_NULL_POINTER;
    if (!d->workspace || d->workspace_bytes < mm_mesh_reg_query_workspace(d)) return MM_ERR_WORKSPACE;
    return MM_OK;
}

size_t mm_mesh_reg_query_workspace(const MMMeshRegDesc* d) {
    if (!d || d->B <= 0 || d->V <= 0 || d->E < 0) return 0;
    return mm::reg_workspace_bytes(d);
}

int mm_mesh_reg_forward(const MMMeshRegDesc* d, mm_stream_t stream) {
    const int st = check_reg(d, false);
    if (st != MM_OK) return st;
    mm::clear_stale_error();
    return mm::launch_reg_fwd(d, (hipStream_t)stream);
}

int mm_mesh_reg_backward(const MMMeshRegDesc* d, const MMMeshRegGrads* g, mm_stream_t stream) {
    const int st = check_reg(d, true);
    if (st != MM_OK) return st;
    if (!g || !g->weights) return MM_ERR_NULL_POINTER;
    if (!g->grad_vertices && !g->grad_delta_vertices && !g->grad_face_normals) return MM_ERR_NULL_POINTER;
    if ((g->grad_vertices && (!d->vertices || !d->sign_init)) || (g->grad_delta_vertices && !d->delta_vertices) ||
        (g->grad_face_normals && !d->face_normals))
        return MM_ERR_NULL_POINTER;                              // a gradient is only defined for an input that was given
    mm::clear_stale_error();
    return mm::launch_reg_bwd(d, g, (hipStream_t)stream);
}

static int check_att(const MMAttLossDesc* d) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->B <= 0 || d->V <= 0 || d->Ht <= 0 || d->Wt <= 0) return MM_ERR_BAD_SHAPE;
    const MMAttributes* two[2] = {&d->pred, &d->target};
    for (const MMAttributes* m : two)
        if (!m->azimuths || !m->elevations || !m->distances || !m->biases || !m->vertices || !m->textures || !m->lights) return MM_ERR_NULL_POINTER;
    if (!d->workspace || d->workspace_bytes < mm_attribute_loss_query_workspace(d)) return MM_ERR_WORKSPACE;
    return MM_OK;
}

size_t mm_attribute_loss_query_workspace(const MMAttLossDesc* d) {
    if (!d || d->B <= 0 || d->Ht <= 0 || d->Wt <= 0) return 0;
    return mm::att_workspace_bytes(d);
}

int mm_attribute_loss_forward(const MMAttLossDesc* d, mm_stream_t stream) {
    const int st = check_att(d);
    if (st != MM_OK) return st;
    if (!d->losses) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_att_fwd(d, (hipStream_t)stream);
}

int mm_attribute_loss_backward(const MMAttLossDesc* d, const MMAttLossGrads* g, mm_stream_t stream) {
    const int st = check_att(d);
    if (st != MM_OK) return st;
    if (!g || !g->weights) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_att_bwd(d, g, (hipStream_t)stream);
}

int mm_disentangle_inputs(const MMDisentangleInputsDesc* d, mm_stream_t stream) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->B <= 0 || d->C <= 0 || d->H <= 0 || d->W <= 0) return MM_ERR_BAD_SHAPE;
    if (d->boxes && d->boxes_rows != d->B) return MM_ERR_BAD_SHAPE;                        // one box per sample, or the batch's one box
    if ((long long)d->B * d->C * d->H * d->W > 0x7fffffffLL) return MM_ERR_UNSUPPORTED;    // the kernels index elements in 32 bits
    if (!d->x || (!d->out_flip && !d->out_erase)) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_disentangle_inputs(d, (hipStream_t)stream);
}

// the flip set and the jitter set are each whole or absent, and each needs its share of Ae
static int check_disentangle(const MMDisentangleDesc* d) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->B <= 0 || d->V <= 0 || d->Ht <= 0 || d->Wt <= 0) return MM_ERR_BAD_SHAPE;
    if ((long long)d->B * 3 * d->Ht * d->Wt > 0x7fffffffLL || (long long)d->B * 3 * d->V > 0x7fffffffLL) return MM_ERR_UNSUPPORTED;
    const bool flip = d->flip_textures || d->flip_vertices;
    const bool jitter = d->jitter_azimuths || d->jitter_elevations || d->jitter_distances || d->jitter_biases || d->jitter_delta_vertices;
    if (flip && (!d->flip_textures || !d->flip_vertices || !d->textures || !d->vertices)) return MM_ERR_NULL_POINTER;
    if (jitter && (!d->jitter_azimuths || !d->jitter_elevations || !d->jitter_distances || !d->jitter_biases || !d->jitter_delta_vertices ||
                   !d->azimuths || !d->elevations || !d->distances || !d->biases || !d->delta_vertices))
        return MM_ERR_NULL_POINTER;
    if (!d->workspace || d->workspace_bytes < mm_disentangle_query_workspace(d)) return MM_ERR_WORKSPACE;
    return MM_OK;
}

size_t mm_disentangle_query_workspace(const MMDisentangleDesc* d) {
    if (!d || d->B <= 0 || d->Ht <= 0 || d->Wt <= 0) return 0;
    return mm::disentangle_workspace_bytes(d);
}

int mm_disentangle_forward(const MMDisentangleDesc* d, mm_stream_t stream) {
    const int st = check_disentangle(d);
    if (st != MM_OK) return st;
    if (!d->terms) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_disentangle_fwd(d, (hipStream_t)stream);
}

int mm_disentangle_backward(const MMDisentangleDesc* d, const MMDisentangleGrads* g, mm_stream_t stream) {
    const int st = check_disentangle(d);
    if (st != MM_OK) return st;
    if (!g || !g->weights) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_disentangle_bwd(d, g, (hipStream_t)stream);
}

static int check_texflow(const MMTexFlowDesc* d) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->B <= 0 || d->C <= 0 || d->H <= 0 || d->W <= 0 || d->Ho <= 0 || d->Wo <= 0) return MM_ERR_BAD_SHAPE;
    if (d->B > 65535 || (d->Ho + 3) / 4 > 65535) return MM_ERR_UNSUPPORTED;     // grid y / z limits
    if (!d->image || !d->flow) return MM_ERR_NULL_POINTER;
    return MM_OK;
}

int mm_texture_flow_forward(const MMTexFlowDesc* d, mm_stream_t stream) {
    const int st = check_texflow(d);
    if (st != MM_OK) return st;
    if (!d->textures) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_texflow_fwd(d, (hipStream_t)stream);
}

int mm_texture_flow_backward(const MMTexFlowDesc* d, const MMTexFlowGrads* g, mm_stream_t stream) {
    const int st = check_texflow(d);
    if (st != MM_OK) return st;
    if (!g || !g->grad_textures || !g->grad_flow) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_texflow_bwd(d, g, (hipStream_t)stream);
}

static bool ssim_shape_ok(const MMSsimDesc* d) {
    if (d->N <= 0 || d->C <= 0 || d->H <= 0 || d->W <= 0 || d->H > 65535 || d->W > 65535) return false;
    if (d->win_size < 1 || d->win_size > MM_SSIM_MAX_WIN || d->win_size % 2 == 0) return false;
    // one workgroup per 64x16 tile of every plane: the grid stays below 2^31 workgroups
    return (int64_t)d->N * d->C * ((d->H + 15) / 16) * ((d->W + 63) / 64) <= 0x7fffffff;
}

size_t mm_ssim_query_workspace(const MMSsimDesc* d) {
    if (!d || !ssim_shape_ok(d)) return 0;
    return mm::ssim_workspace_bytes(d);
}

static int check_ssim(const MMSsimDesc* d) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (!ssim_shape_ok(d)) return MM_ERR_BAD_SHAPE;
    if (!d->x || !d->y) return MM_ERR_NULL_POINTER;
    if (!d->workspace || d->workspace_bytes < mm::ssim_workspace_bytes(d)) return MM_ERR_WORKSPACE;
    return MM_OK;
}

int mm_ssim_forward(const MMSsimDesc* d, mm_stream_t stream) {
    const int st = check_ssim(d);
    if (st != MM_OK) return st;
    if (!d->ssim) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_ssim_fwd(d, (hipStream_t)stream);
}

int mm_ssim_backward(const MMSsimDesc* d, const MMSsimGrads* g, mm_stream_t stream) {
    const int st = check_ssim(d);
    if (st != MM_OK) return st;
    if (!g || (!g->grad_ssim && !g->grad_cs) || (!g->grad_x && !g->grad_y)) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_ssim_bwd(d, g, (hipStream_t)stream);
}

// the sizes both encoder-feature ops share: one workgroup per (b, c) plane, one LDS float per vertex, int32 pixel indices
static bool encfeat_shape_ok(int B, int C, int H, int W, int V, int dtype) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || V <= 0 || V > MM_ENCFEAT_MAX_V) return false;
    if (dtype != MM_DTYPE_F32 && dtype != MM_DTYPE_F16 && dtype != MM_DTYPE_BF16) return false;
    return (int64_t)B * C <= 0x7fffffff && (int64_t)H * W <= (1 << 30);
}

static bool shape_feat_ok(const MMShapeFeatDesc* d) {
    return encfeat_shape_ok(d->B, d->C, d->H, d->W, d->V, d->x_dtype) && d->col_k >= 1 && d->col_k <= d->V && d->row_k >= 1 &&
           d->row_k <= d->V;
}

size_t mm_shape_features_query_workspace(const MMShapeFeatDesc* d) {
    if (!d || !shape_feat_ok(d)) return 0;
    return mm::encfeat_workspace_bytes(d->B, d->C, d->H, d->W, d->V, 1);
}

int mm_shape_features_forward(const MMShapeFeatDesc* d, mm_stream_t stream) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (!shape_feat_ok(d)) return MM_ERR_BAD_SHAPE;
    if (!d->x || !d->template_xyz || !d->col_idx || !d->col_val || !d->p || !d->out) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_shape_feat_fwd(d, (hipStream_t)stream);
}

int mm_shape_features_backward(const MMShapeFeatDesc* d, const MMShapeFeatGrads* g, mm_stream_t stream) {
    if (!d || !g) return MM_ERR_NULL_POINTER;
    if (!shape_feat_ok(d)) return MM_ERR_BAD_SHAPE;
    if (!d->x || !d->template_xyz || !d->row_idx || !d->row_val || !d->p || !g->grad_out || (!g->grad_x && !g->grad_p))
        return MM_ERR_NULL_POINTER;
    if (!d->workspace || d->workspace_bytes < mm_shape_features_query_workspace(d)) return MM_ERR_WORKSPACE;
    mm::clear_stale_error();
    return mm::launch_shape_feat_bwd(d, g, (hipStream_t)stream);
}

size_t mm_camera_features_query_workspace(const MMCameraFeatDesc* d) {
    if (!d || !encfeat_shape_ok(d->B, d->C, d->H, d->W, d->V, d->x_dtype)) return 0;
    return mm::encfeat_workspace_bytes(d->B, d->C, d->H, d->W, d->V, 2);
}

int mm_camera_features_forward(const MMCameraFeatDesc* d, mm_stream_t stream) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (!encfeat_shape_ok(d->B, d->C, d->H, d->W, d->V, d->x_dtype)) return MM_ERR_BAD_SHAPE;
    if (!d->x || !d->template_xyz || !d->p_map || !d->p_local || !d->out) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_camera_feat_fwd(d, (hipStream_t)stream);
}

int mm_camera_features_backward(const MMCameraFeatDesc* d, const MMCameraFeatGrads* g, mm_stream_t stream) {
    if (!d || !g) return MM_ERR_NULL_POINTER;
    if (!encfeat_shape_ok(d->B, d->C, d->H, d->W, d->V, d->x_dtype)) return MM_ERR_BAD_SHAPE;
    if (!d->x || !d->template_xyz || !d->p_map || !d->p_local || !g->grad_out || (!g->grad_x && !g->grad_p_map && !g->grad_p_local))
        return MM_ERR_NULL_POINTER;
    if (!d->workspace || d->workspace_bytes < mm_camera_features_query_workspace(d)) return MM_ERR_WORKSPACE;
    mm::clear_stale_error();
    return mm::launch_camera_feat_bwd(d, g, (hipStream_t)stream);
}

// sizes of the attribute mix: every row length and the launch's chunk count (one chunk per <= 1024 floats of a row) fit an int32
// has_bg: the forward's bg, or the backward's bg gradient pair (the backward reads no source)
static int interp_shape(const MMInterpDesc* d, bool has_bg) {
    if (d->B <= 0 || d->V <= 0 || d->Ht <= 0 || d->Wt <= 0 || (has_bg && (d->H <= 0 || d->W <= 0))) return MM_ERR_BAD_SHAPE;
    if (d->B > 65535) return MM_ERR_UNSUPPORTED;
    const int64_t lens[3] = {3LL * d->V, 3LL * d->Ht * d->Wt, has_bg ? 3LL * d->H * d->W : 0};
    int64_t chunks = 2 * (lens[0] / 1024 + 1) + 1;
    for (int t = 1; t < 3; ++t) {
        if (lens[t] > 0x7fffffff) return MM_ERR_UNSUPPORTED;
        chunks += lens[t] / 1024 + 1;
    }
    return chunks * d->B > 0x7fffffff ? MM_ERR_UNSUPPORTED : MM_OK;
}

size_t mm_interp_query_workspace(const MMInterpDesc* d) {
    if (!d || interp_shape(d, false) != MM_OK) return 0;
    return mm::interp_workspace_bytes(d->B);
}

int mm_attribute_mix_forward(const MMInterpDesc* d, mm_stream_t stream) {
    if (!d) return MM_ERR_NULL_POINTER;
    const int st = interp_shape(d, d->bg != nullptr);
    if (st != MM_OK) return st;
    if (!d->vertices || !d->delta_vertices || !d->textures || !d->lights || !d->out_vertices || !d->out_delta_vertices ||
        !d->out_textures || !d->out_lights || (d->bg && !d->out_bg) || !d->idx_a || !d->idx_b || !d->alpha_shape || !d->alpha_texture ||
        !d->alpha_light)
        return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_mix_fwd(d, (hipStream_t)stream);
}

int mm_attribute_mix_backward(const MMInterpDesc* d, const MMInterpGrads* g, mm_stream_t stream) {
    if (!d || !g) return MM_ERR_NULL_POINTER;
    const int st = interp_shape(d, g->grad_out_bg || g->grad_bg);
    if (st != MM_OK) return st;
    if (!d->idx_a || !d->idx_b || !d->alpha_shape || !d->alpha_texture || !d->alpha_light) return MM_ERR_NULL_POINTER;
    const void* up[5] = {g->grad_out_vertices, g->grad_out_delta_vertices, g->grad_out_textures, g->grad_out_bg, g->grad_out_lights};
    const void* gs[5] = {g->grad_vertices, g->grad_delta_vertices, g->grad_textures, g->grad_bg, g->grad_lights};
    bool any = false;
    for (int t = 0; t < 5; ++t) {
        if (!up[t] != !gs[t]) return MM_ERR_NULL_POINTER;     // an upstream gradient without its destination, or the reverse
        any = any || up[t];
    }
    if (!any) return MM_OK;                                   // nothing to differentiate: nothing is launched
    if (!d->workspace || d->workspace_bytes < mm_interp_query_workspace(d)) return MM_ERR_WORKSPACE;
    mm::clear_stale_error();
    return mm::launch_mix_bwd(d, g, (hipStream_t)stream);
}

int mm_collapse_resample(int32_t B, int32_t V, const float* delta_vertices, int32_t* idx_a, int32_t* idx_b, const float* uniforms,
                         float threshold, int32_t* n_bad, mm_stream_t stream) {
    if (!delta_vertices || !idx_a || !idx_b || !uniforms || !n_bad) return MM_ERR_NULL_POINTER;
    if (B <= 0 || V <= 0) return MM_ERR_BAD_SHAPE;
    if (B > 65535) return MM_ERR_UNSUPPORTED;                     // the good mask lives in LDS: one bit per sample
    mm::clear_stale_error();
    return mm::launch_collapse_resample(B, V, delta_vertices, idx_a, idx_b, uniforms, threshold, n_bad, (hipStream_t)stream);
}

// sizes and modes of the critic inputs; the launches count chunks of one image in an int32 (two fakes in the backward)
static int critic_shape(const MMCriticDesc* d) {
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->unmask < 0 || d->unmask > 2) return MM_ERR_BAD_SHAPE;
    if (!d->alpha_er90 != !d->alpha_ir) return MM_ERR_BAD_SHAPE;  // one interpolate without the other
    if (2LL * d->B * mm::critic_chunks_per_image(d) > 0x7fffffff) return MM_ERR_UNSUPPORTED;
    return MM_OK;
}

int mm_critic_inputs_forward(const MMCriticDesc* d, mm_stream_t stream) {
    if (!d) return MM_ERR_NULL_POINTER;
    const int st = critic_shape(d);
    if (st != MM_OK) return st;
    if (!d->Xa || !d->Xer90 || !d->Xir || !d->out_batch || (d->alpha_er90 && (!d->out_gp_er90 || !d->out_gp_ir))) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_critic_fwd(d, (hipStream_t)stream);
}

int mm_critic_inputs_backward(const MMCriticDesc* d, const MMCriticGrads* g, mm_stream_t stream) {
    if (!d || !g) return MM_ERR_NULL_POINTER;
    const int st = critic_shape(d);
    if (st != MM_OK) return st;
    if (!g->grad_er90 && !g->grad_ir) return MM_OK;            // nothing to differentiate: nothing is launched
    if (!g->g_batch) return MM_ERR_NULL_POINTER;
    if (d->unmask == 0 && ((g->grad_er90 && !d->Xer90) || (g->grad_ir && !d->Xir))) return MM_ERR_NULL_POINTER;   // d m reads the fake
    mm::clear_stale_error();
    return mm::launch_critic_bwd(d, g, (hipStream_t)stream);
}

// sizes and modes the two exports share
static int export_shape(const MMExportDesc* d) {
    if (d->B <= 0 || d->N <= 0 || d->H <= 0 || d->W <= 0 || (d->C != 3 && d->C != 4)) return MM_ERR_BAD_SHAPE;
    if (d->C == 3 && (d->white || d->nhwc)) return MM_ERR_BAD_SHAPE;
    if (d->rounding != 0 && d->rounding != 1) return MM_ERR_BAD_SHAPE;
    return MM_OK;
}

int mm_export_images(const MMExportDesc* d, mm_stream_t stream) {
    if (!d) return MM_ERR_NULL_POINTER;
    const int st = export_shape(d);
    if (st != MM_OK) return st;
    if (!d->out_rgb && !d->out_mask && !d->out_rgba) return MM_ERR_BAD_SHAPE;     // no output requested
    if (d->C == 3 && (d->out_mask || d->out_rgba)) return MM_ERR_BAD_SHAPE;
    // groups of 16 pixels are counted in an int32
    const long long images = (long long)d->B * d->N, HW = (long long)d->H * d->W;
    if (images > (0x7fffffffLL * 16) / HW) return MM_ERR_UNSUPPORTED;
    if (!d->x) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_export_images(d, (hipStream_t)stream);
}

int mm_export_grid(const MMExportDesc* d, mm_stream_t stream) {
    if (!d) return MM_ERR_NULL_POINTER;
    const int st = export_shape(d);
    if (st != MM_OK) return st;
    if (d->nrow < 1 || d->padding < 0) return MM_ERR_BAD_SHAPE;
    long long xmaps, pad, Hg, Wg;
    mm::export_grid_geometry(d, &xmaps, &pad, &Hg, &Wg);
    const long long chunks = 0x7fffffffLL - 32;                   // 16-byte chunks of the sheets, and 32 items for the bytes around them
    if (Hg > 0x7fffffffLL || Wg > 0x7fffffffLL || Hg > chunks * 16 / 3 / Wg || (long long)d->N > chunks * 16 / 3 / (Hg * Wg)) return MM_ERR_UNSUPPORTED;
    if (!d->x || !d->out_grid) return MM_ERR_NULL_POINTER;
    mm::clear_stale_error();
    return mm::launch_export_grid(d, (hipStream_t)stream);
}

int mm_assemble_batch(const MMBatchDesc* d, mm_stream_t stream) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (!d->images || !d->segs || !d->offsets || !d->sizes || !d->records_host || !d->records || !d->out) return MM_ERR_NULL_POINTER;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->n_images <= 0) return MM_ERR_BAD_SHAPE;
    const int32_t lim = 1 << 24;                                  // sums of two coordinates stay far inside an int32
    for (int b = 0; b < d->B; ++b) {
        const int32_t* r = d->records_host + (size_t)b * 16;
        if (r[0] < 0 || r[0] >= d->n_images || r[4] < 1 || r[5] < 1 || r[10] < 1 || r[11] < 1) return MM_ERR_BAD_SHAPE;
        if ((r[1] != 0 && r[1] != 1) || (r[14] != 0 && r[14] != 1)) return MM_ERR_BAD_SHAPE;
        for (int i = 2; i < 14; ++i)
            if (r[i] > lim || r[i] < -lim) return MM_ERR_BAD_SHAPE;
    }
    if (d->B > 65535) return MM_ERR_UNSUPPORTED;
    for (int b = 0; b < d->B; ++b) {
        const int32_t* r = d->records_host + (size_t)b * 16;
        if (r[4] > (int64_t)MM_BATCH_MAX_RATIO * r[10] || r[5] > (int64_t)MM_BATCH_MAX_RATIO * r[11]) return MM_ERR_UNSUPPORTED;
    }
    if (mm::batch_lds_bytes(d, nullptr) > 160 * 1024) return MM_ERR_UNSUPPORTED;
    mm::clear_stale_error();
    return mm::launch_assemble_batch(d, (hipStream_t)stream);
}

int mm_composite_frames(const MMCompositeDesc* d, mm_stream_t stream) {
    const int st = check_frames(d);
    if (st != MM_OK) return st;
    const int32_t ks[2] = {d->mask_k, d->bg_k};
    for (int i = 0; i < 2; ++i)
        if (ks[i] < 1 || ks[i] > MM_COMPOSITE_MAX_KERNEL || !(ks[i] & 1)) return MM_ERR_BAD_SHAPE;
    if (d->mask_pad < 0 || d->mask_pad > (1 << 24)) return MM_ERR_BAD_SHAPE;
    // ... and the blur radius narrower than what it reflects in
    const int32_t* bp = d->bg_pad;
    const int32_t Hp = d->H + bp[2] + bp[3], Wp = d->W + bp[0] + bp[1];
    if (d->mask_k / 2 >= d->H || d->mask_k / 2 >= d->W || d->bg_k / 2 >= Hp || d->bg_k / 2 >= Wp) return MM_ERR_BAD_SHAPE;
    const int32_t* row = d->params_host + 2 * (size_t)d->B + (size_t)d->B * d->mask_k + (size_t)d->B * d->bg_k;
    const int32_t n_out[4] = {d->H, d->W, d->H, d->W};
    const int32_t n_in[4] = {d->H + 2 * d->mask_pad, d->W + 2 * d->mask_pad, Hp, Wp};
    for (int t = 0; t < 4; ++t)
        if (check_resize_rows(row, n_out[t], n_in[t]) != MM_OK) return MM_ERR_BAD_SHAPE;
    if (mm::composite_lds_bytes(d, nullptr) > 160 * 1024) return MM_ERR_UNSUPPORTED;
    if ((long long)d->B * ((d->H + MM_COMPOSITE_ROWS - 1) / MM_COMPOSITE_ROWS) > 0x7fffffffLL) return MM_ERR_UNSUPPORTED;
    mm::clear_stale_error();
    return mm::launch_composite(d, (hipStream_t)stream);
}

int mm_pyramid_frames(const MMPyramidDesc* d, mm_stream_t stream) {
    const int st = check_frames(d);
    if (st != MM_OK) return st;
    if (d->k < 1 || d->k > MM_PYRAMID_MAX_KERNEL || !(d->k & 1) || d->B > (1 << 24)) return MM_ERR_BAD_SHAPE;
    if (d->k / 2 >= d->H || d->k / 2 >= d->W) return MM_ERR_BAD_SHAPE;     // ... and so is the blur radius, at every level
    const int32_t* bp = d->bg_pad;
    const int32_t* row = d->params_host + 2 * (size_t)d->B + 9 * (size_t)d->B * d->k;
    if (check_resize_rows(row, d->H, d->H + bp[2] + bp[3]) != MM_OK || check_resize_rows(row, d->W, d->W + bp[0] + bp[1]) != MM_OK) return MM_ERR_BAD_SHAPE;
    if (mm::pyramid_lds_bytes(d, nullptr) > 160 * 1024) return MM_ERR_UNSUPPORTED;
    if ((long long)d->B * ((d->H + MM_PYRAMID_ROWS - 1) / MM_PYRAMID_ROWS) > 0x7fffffffLL) return MM_ERR_UNSUPPORTED;
    mm::clear_stale_error();
    return mm::launch_pyramid(d, (hipStream_t)stream);
}

int mm_poisson_frames(const MMPoissonDesc* d, mm_stream_t stream) {
    const int st = check_frames(d);
    if (st != MM_OK) return st;
    if ((d->border != 0 && d->border != 1) || d->B > (1 << 24)) return MM_ERR_BAD_SHAPE;
    if (d->sweeps < 0 || d->sweeps > MM_POISSON_MAX_SWEEPS || !(d->omega > 0.0f && d->omega < 2.0f)) return MM_ERR_BAD_SHAPE;
    const int32_t* bp = d->bg_pad;
    const int32_t* row = d->params_host + 2 * (size_t)d->B;
    if (check_resize_rows(row, d->H, d->H + bp[2] + bp[3]) != MM_OK || check_resize_rows(row, d->W, d->W + bp[0] + bp[1]) != MM_OK) return MM_ERR_BAD_SHAPE;
    if (mm::poisson_lds_bytes(d, nullptr) > 160 * 1024) return MM_ERR_UNSUPPORTED;
    mm::clear_stale_error();
    return mm::launch_poisson(d, (hipStream_t)stream);
}

// the sizes a JPEG call may have: MM_OK, or why not
static int check_jpeg_shape(const MMJpegModesDesc* d) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->n <= 0 || d->H <= 0 || d->W <= 0 || d->header_bytes < 2 || d->header_bytes > MM_JPEG_MAX_HEADER) return MM_ERR_BAD_SHAPE;
    const int layout = mm::jpeg_layout_of(d->mode, d->sampling);
    if (layout < 0) return MM_ERR_BAD_SHAPE;
    if (d->H > 65535 || d->W > 65535 || d->n > 65535) return MM_ERR_UNSUPPORTED;
    const long long blocks = mm::jpeg_frame_blocks(d->H, d->W, layout);     // the layout's own: 6, 4, 3 or 1 per MCU
    if (blocks > MM_JPEG_MAX_BLOCKS || blocks * d->n > (1LL << 30)) return MM_ERR_UNSUPPORTED;
    return MM_OK;
}

size_t mm_jpeg_modes_query_workspace(const MMJpegModesDesc* d) {
    return check_jpeg_shape(d) == MM_OK ? mm::jpeg_workspace_bytes(d) : 0;
}

size_t mm_jpeg_modes_files_offset(const MMJpegModesDesc* d) {
    return check_jpeg_shape(d) == MM_OK ? mm::jpeg_files_at(d) : 0;
}

size_t mm_jpeg_modes_coef_offset(const MMJpegModesDesc* d) {
    return check_jpeg_shape(d) == MM_OK ? mm::jpeg_coef_at(d) : 0;
}

int mm_jpeg_modes_encode(const MMJpegModesDesc* d, mm_stream_t stream) {
    const int shape = check_jpeg_shape(d);
    if (shape != MM_OK) return shape;
    if (!d->frames || !d->params_host || !d->params || !d->workspace) return MM_ERR_NULL_POINTER;
    if (d->workspace_bytes < mm::jpeg_workspace_bytes(d) || ((uintptr_t)d->workspace & 15)) return MM_ERR_WORKSPACE;
    const int32_t* par = d->params_host;
    for (int i = 0; i < 128; ++i)                                 // the divisors: 8 * q, q in 1..255 (baseline)
        if (par[i] < 8 || par[i] > 8 * 255 || (par[i] & 7)) return MM_ERR_BAD_SHAPE;
    for (int i = 0; i < 1024; ++i) {                              // the codes: at most 16 bits, no wider than their size, and with the symbol's
        const uint32_t size = (uint32_t)par[128 + i] >> 16, code = (uint32_t)par[128 + i] & 0xFFFFu;      // category bits at most 26: a block's room
        if (size > 16 || (code >> size) != 0 || (size != 0 && size + (i & 15) > 26)) return MM_ERR_BAD_SHAPE;
    }
    mm::clear_stale_error();
    return mm::launch_jpeg(d, (hipStream_t)stream);
}

// MMJpegDesc is MMJpegModesDesc with mode RGB and sampling 4:2:0: mm_jpeg_* forward
static const MMJpegModesDesc* jpeg_as_modes(const MMJpegDesc* d, MMJpegModesDesc* e) {
    if (!d) return nullptr;
    *e = MMJpegModesDesc{};
    e->n = d->n; e->H = d->H; e->W = d->W; e->header_bytes = d->header_bytes;
    e->mode = MM_JPEG_MODE_RGB; e->sampling = MM_JPEG_SAMPLING_420;
    e->frames = d->frames; e->params_host = d->params_host; e->params = d->params;
    e->workspace = d->workspace; e->workspace_bytes = d->workspace_bytes;
    return e;
}

size_t mm_jpeg_query_workspace(const MMJpegDesc* d) {
    MMJpegModesDesc e;
    return mm_jpeg_modes_query_workspace(jpeg_as_modes(d, &e));
}

size_t mm_jpeg_files_offset(const MMJpegDesc* d) {
    MMJpegModesDesc e;
    return mm_jpeg_modes_files_offset(jpeg_as_modes(d, &e));
}

int mm_jpeg_encode(const MMJpegDesc* d, mm_stream_t stream) {
    MMJpegModesDesc e;
    return mm_jpeg_modes_encode(jpeg_as_modes(d, &e), stream);
}

size_t mm_jpeg_coef_offset(const MMJpegDesc* d) {
    MMJpegModesDesc e;
    return mm_jpeg_modes_coef_offset(jpeg_as_modes(d, &e));
}

// the sizes a round trip may have: the encoder's, in both modes
static int check_jpeg_roundtrip_shape(const MMJpegRoundtripDesc* d) {
    if (!d) return MM_ERR_NULL_POINTER;
    MMJpegModesDesc e = {};                                       // (an unknown mode or sampling, or a sampling with mode L: refused there)
    e.n = d->n; e.H = d->H; e.W = d->W; e.header_bytes = 2; e.mode = d->mode; e.sampling = d->sampling;
    return check_jpeg_shape(&e);
}

size_t mm_jpeg_roundtrip_query_workspace(const MMJpegRoundtripDesc* d) {
    return check_jpeg_roundtrip_shape(d) == MM_OK ? mm::jpeg_roundtrip_workspace_bytes(d) : 0;
}

int mm_jpeg_roundtrip(const MMJpegRoundtripDesc* d, mm_stream_t stream) {
    const int shape = check_jpeg_roundtrip_shape(d);
    if (shape != MM_OK) return shape;
    const bool rgb = d->mode == MM_JPEG_MODE_RGB;
    if (!d->params_host || !d->params || !d->out || (!d->frames && !(rgb && d->coef)) || (rgb && !d->workspace)) return MM_ERR_NULL_POINTER;
    if (rgb && (d->workspace_bytes < mm::jpeg_roundtrip_workspace_bytes(d) || ((uintptr_t)d->workspace & 15) || ((uintptr_t)d->coef & 15))) return MM_ERR_WORKSPACE;
    if ((uintptr_t)d->out & 3) return MM_ERR_WORKSPACE;
    for (int i = 0; i < 128; ++i)                                 // the divisors: 8 * q, q in 1..255 (baseline)
        if (d->params_host[i] < 8 || d->params_host[i] > 8 * 255 || (d->params_host[i] & 7)) return MM_ERR_BAD_SHAPE;
    mm::clear_stale_error();
    return mm::launch_jpeg_roundtrip(d, (hipStream_t)stream);
}

// the sizes a GIF call may have: MM_OK, or why not
static int check_gif_shape(const MMGifDesc* d) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->n <= 0 || d->H <= 0 || d->W <= 0 || d->segment < 1 || d->segment > MM_GIF_MAX_SEGMENT) return MM_ERR_BAD_SHAPE;
    if (d->delay < 0 || d->delay > 65535 || d->loop < -1 || d->loop > 65535) return MM_ERR_BAD_SHAPE;
    if (d->H > 65535 || d->W > 65535 || d->n > 65535) return MM_ERR_UNSUPPORTED;
    if ((long long)d->n * d->H * d->W >= (1LL << 29)) return MM_ERR_UNSUPPORTED;         // 7 * count stays inside 32 bits
    return MM_OK;
}

size_t mm_gif_query_workspace(const MMGifDesc* d) {
    return check_gif_shape(d) == MM_OK ? mm::gif_workspace_bytes(d) : 0;
}

size_t mm_gif_file_offset(const MMGifDesc* d) {
    return check_gif_shape(d) == MM_OK ? mm::gif_file_at(d) : 0;
}

int mm_gif_encode(const MMGifDesc* d, mm_stream_t stream) {
    const int shape = check_gif_shape(d);
    if (shape != MM_OK) return shape;
    if (!d->frames || !d->palette || !d->indices || !d->workspace) return MM_ERR_NULL_POINTER;
    if (d->workspace_bytes < mm::gif_workspace_bytes(d) || ((uintptr_t)d->workspace & 15)) return MM_ERR_WORKSPACE;
    mm::clear_stale_error();
    return mm::launch_gif(d, (hipStream_t)stream);
}

// the sizes a PNG call may have: MM_OK, or why not
static int check_png_shape(const MMPngDesc* d) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->n <= 0 || d->H <= 0 || d->W <= 0 || (d->channels != 1 && d->channels != 3 && d->channels != 4)) return MM_ERR_BAD_SHAPE;
    if (d->filter < -1 || d->filter > 4 || d->segment < 1 || d->segment > MM_PNG_MAX_SEGMENT) return MM_ERR_BAD_SHAPE;
    if (d->H > 65535 || d->W > 65535 || d->n > 65535) return MM_ERR_UNSUPPORTED;
    if (mm::png_idat_cap(d) > 0x7fffffffLL || mm::png_all_segs(d) > 0x7fffffffLL) return MM_ERR_UNSUPPORTED;      // a chunk's length; the grids
    return MM_OK;
}

size_t mm_png_query_workspace(const MMPngDesc* d) {
    return check_png_shape(d) == MM_OK ? mm::png_workspace_bytes(d) : 0;
}

size_t mm_png_files_offset(const MMPngDesc* d) {
    return check_png_shape(d) == MM_OK ? mm::png_files_at(d) : 0;
}

int mm_png_encode(const MMPngDesc* d, mm_stream_t stream) {
    const int shape = check_png_shape(d);
    if (shape != MM_OK) return shape;
    if (!d->frames || !d->workspace) return MM_ERR_NULL_POINTER;
    if (d->workspace_bytes < mm::png_workspace_bytes(d) || ((uintptr_t)d->workspace & 15)) return MM_ERR_WORKSPACE;
    mm::clear_stale_error();
    return mm::launch_png(d, (hipStream_t)stream);
}

size_t mm_jpeg_decode_query_workspace(const MMJpegDecodeDesc* d) {
    return mm::check_jpeg_decode(d) == MM_OK ? mm::jpeg_decode_workspace_bytes(d) : 0;
}

int mm_jpeg_decode(const MMJpegDecodeDesc* d, mm_stream_t stream) {
    const int shape = mm::check_jpeg_decode(d);                   // (every record of tables_host: csrc/mm_jpeg_decode.hip)
    if (shape != MM_OK) return shape;
    if (!d->bytes || !d->tables || !d->out || !d->workspace) return MM_ERR_NULL_POINTER;
    if (d->workspace_bytes < mm::jpeg_decode_workspace_bytes(d) || ((uintptr_t)d->workspace & 15) || ((uintptr_t)d->tables & 15)) return MM_ERR_WORKSPACE;
    mm::clear_stale_error();
    return mm::launch_jpeg_decode(d, (hipStream_t)stream);
}

size_t mm_png_decode_query_workspace(const MMPngDecodeDesc* d) {
    return mm::check_png_decode(d) == MM_OK ? mm::png_decode_workspace_bytes(d) : 0;
}

int mm_png_decode(const MMPngDecodeDesc* d, mm_stream_t stream) {
    const int shape = mm::check_png_decode(d);                    // (every record of tables_host: csrc/mm_png_decode.hip)
    if (shape != MM_OK) return shape;
    if (!d->bytes || !d->tables || !d->out || !d->workspace) return MM_ERR_NULL_POINTER;
    if (d->workspace_bytes < mm::png_decode_workspace_bytes(d) || ((uintptr_t)d->workspace & 15) || ((uintptr_t)d->tables & 15)) return MM_ERR_WORKSPACE;
    mm::clear_stale_error();
    return mm::launch_png_decode(d, (hipStream_t)stream);
}

int mm_fid_input(const MMFidInputDesc* d, mm_stream_t stream) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->n <= 0 || d->H < 1 || d->W < 1 || d->Ho < 1 || d->Wo < 1) return MM_ERR_BAD_SHAPE;
    if (d->H > MM_FID_MAX_SIDE || d->W > MM_FID_MAX_SIDE || d->Ho > MM_FID_MAX_SIDE || d->Wo > MM_FID_MAX_SIDE) return MM_ERR_BAD_SHAPE;
    if (!d->frames || !d->params_host || !d->params || !d->out) return MM_ERR_NULL_POINTER;
    if ((uintptr_t)d->params & 15) return MM_ERR_BAD_SHAPE;
    if ((long long)d->n * ((d->Ho + 7) / 8) > 0x7fffffffLL) return MM_ERR_UNSUPPORTED;
    const int32_t* row = d->params_host;                          // every tap inside its axis, before anything is launched
    for (int i = 0; i < d->Wo + d->Ho; ++i, row += 4) {
        const int32_t n_in = i < d->Wo ? d->W : d->H;
        if (row[0] < 0 || row[0] >= n_in || row[1] < 0 || row[1] >= n_in) return MM_ERR_BAD_SHAPE;
    }
    mm::clear_stale_error();
    return mm::launch_fid_input(d, (hipStream_t)stream);
}

// the sizes a statistics call may have: MM_OK, or why not
static int check_fid_stats_shape(const MMFidStatsDesc* d) {
    if (!d) return MM_ERR_NULL_POINTER;
    if (d->N < 2 || d->D < 1) return MM_ERR_BAD_SHAPE;
    if (d->D > 65535 || d->N > 65535 * MM_FID_SUM_ROWS) return MM_ERR_UNSUPPORTED;      // the grids' y and the tile count
    return MM_OK;
}

size_t mm_fid_stats_query_workspace(const MMFidStatsDesc* d) {
    return check_fid_stats_shape(d) == MM_OK ? mm::fid_stats_workspace_bytes(d) : 0;
}

int mm_fid_stats(const MMFidStatsDesc* d, mm_stream_t stream) {
    const int shape = check_fid_stats_shape(d);
    if (shape != MM_OK) return shape;
    if (!d->x || !d->mu || !d->sigma || !d->workspace) return MM_ERR_NULL_POINTER;
    if (d->workspace_bytes < mm::fid_stats_workspace_bytes(d) || ((uintptr_t)d->workspace & 255)) return MM_ERR_WORKSPACE;
    mm::clear_stale_error();
    return mm::launch_fid_stats(d, (hipStream_t)stream);
}

int mm_build_vertex_corner_csr(int32_t V, int32_t F, const int32_t* faces, int32_t* offsets, int32_t* items) {
    if (!faces || !offsets || !items) return MM_ERR_NULL_POINTER;
    if (V <= 0 || F <= 0) return MM_ERR_BAD_SHAPE;
    for (int i = 0; i <= V; ++i) offsets[i] = 0;
    for (int i = 0; i < 3 * F; ++i) {
        if (faces[i] < 0 || faces[i] >= V) return MM_ERR_BAD_SHAPE;
        ++offsets[faces[i] + 1];
    }
    for (int i = 0; i < V; ++i) offsets[i + 1] += offsets[i];
    // counting sort: corners visited ascending, so each vertex's list is ascending; offsets doubles as the cursor
    for (int i = 0; i < 3 * F; ++i) items[offsets[faces[i]]++] = i;
    for (int v = V; v > 0; --v) offsets[v] = offsets[v - 1];
    offsets[0] = 0;
    return MM_OK;
}

int mm_build_vertex_corner_table(int32_t V, int32_t F, const int32_t* faces, int32_t stride, int32_t* table) {
    if (!faces) return MM_ERR_NULL_POINTER;
    if (V <= 0 || F <= 0) return MM_ERR_BAD_SHAPE;
    int32_t* cnt = (int32_t*)calloc((size_t)V, sizeof(int32_t));                 // (a host helper: the GPU path never allocates)
    if (!cnt) return MM_ERR_WORKSPACE;
    int32_t valence = 0;
    for (int i = 0; i < 3 * F; ++i) {
        if (faces[i] < 0 || faces[i] >= V) { free(cnt); return MM_ERR_BAD_SHAPE; }
        if (++cnt[faces[i]] > valence) valence = cnt[faces[i]];
    }
    if (!table) { free(cnt); return valence; }
    if (stride < valence) { free(cnt); return MM_ERR_BAD_SHAPE; }
    for (size_t i = 0; i < (size_t)V * stride * 4; ++i) table[i] = -1;
    for (int v = 0; v < V; ++v) cnt[v] = 0;
    for (int i = 0; i < 3 * F; ++i) {                             // corners visited ascending: every vertex's list is ascending
        const int v = faces[i], f = i / 3;
        int32_t* e = table + ((size_t)v * stride + cnt[v]++) * 4;
        e[0] = i; e[1] = faces[f * 3]; e[2] = faces[f * 3 + 1]; e[3] = faces[f * 3 + 2];
    }
    free(cnt);
    return MM_OK;
}

const char* mm_status_string(int status) {
    switch (status) {
        case MM_OK: return "ok";
        case MM_ERR_NULL_POINTER: return "required pointer is NULL";
        case MM_ERR_BAD_SHAPE: return "bad or inconsistent size";
        case MM_ERR_WORKSPACE: return "workspace missing, misaligned or too small";
        case MM_ERR_LAUNCH: return "HIP launch failed";
        case MM_ERR_UNSUPPORTED: return "unsupported option";
        default: return "unknown status";
    }
}

const char* mm_last_error_detail(void) {
    static thread_local char buf[160];
    const mm::LaunchError& e = mm::last_launch_error();
    if (e.code == hipSuccess) return "";
    snprintf(buf, sizeof buf, "%s: %s (hipError %d)", e.what, hipGetErrorString(e.code), (int)e.code);
    return buf;
}

size_t mm_struct_size(int which) {
    switch (which) {
        case 0: return sizeof(MMRenderDesc);    case 1: return sizeof(MMRenderGrads);   case 2: return sizeof(MMReconDesc);
        case 3: return sizeof(MMMeshRegDesc);   case 4: return sizeof(MMMeshRegGrads);  case 5: return sizeof(MMAttLossDesc);
        case 6: return sizeof(MMAttLossGrads);  case 7: return sizeof(MMTexFlowDesc);   case 8: return sizeof(MMTexFlowGrads);
        case 9: return sizeof(MMPrepareDesc);   case 10: return sizeof(MMPrepareGrads); case 11: return sizeof(MMDibrDesc);
        case 12: return sizeof(MMDibrGrads);    case 13: return sizeof(MMTexMapDesc);   case 14: return sizeof(MMTexMapGrads);
        case 15: return sizeof(MMShDesc);       case 16: return sizeof(MMShGrads);      case 17: return sizeof(MMMaskIouDesc);
        case 18: return sizeof(MMSsimDesc);     case 19: return sizeof(MMSsimGrads);    case 20: return sizeof(MMShapeFeatDesc);
        case 21: return sizeof(MMShapeFeatGrads); case 22: return sizeof(MMCameraFeatDesc); case 23: return sizeof(MMCameraFeatGrads);
        case 24: return sizeof(MMInterpDesc);   case 25: return sizeof(MMInterpGrads);  case 26: return sizeof(MMRenderViewsDesc);
        case 27: return sizeof(MMCriticDesc);   case 28: return sizeof(MMCriticGrads);  case 29: return sizeof(MMExportDesc);
        case 30: return sizeof(MMBatchDesc);    case 32: return sizeof(MMCompositeDesc);   // (31: unassigned)
        case 33: return sizeof(MMRenderIndexedDesc); case 35: return sizeof(MMPyramidDesc);     // (34: unassigned)
        case 37: return sizeof(MMJpegDesc);     case 38: return sizeof(MMJpegRoundtripDesc);    // (36: unassigned)
        case 39: return sizeof(MMGifDesc); case 40: return sizeof(MMPoissonDesc); case 41: return sizeof(MMPngDesc);
        case 42: return sizeof(MMJpegModesDesc); case 43: return sizeof(MMFidInputDesc); case 44: return sizeof(MMFidStatsDesc);
        case 45: return sizeof(MMJpegDecodeDesc); case 46: return sizeof(MMPngDecodeDesc);
        case 47: return sizeof(MMDisentangleInputsDesc); case 48: return sizeof(MMDisentangleDesc); case 49: return sizeof(MMDisentangleGrads);
        default: return 0;
    }
}

int mm_abi_version(void) { return MM_ABI_VERSION; }

}  // extern "C"
