/*
 * mm_render.h -- C ABI of libmm_render.so: the MI355X (gfx950) differentiable render + reconstruction-loss path of
 * 3D-Magic-Mirror.
 *
 * This is the drop-in boundary for the path
 *     DiffRender.render        /root/reference/networks.py:258-324
 *     DiffRender.recon_data    /root/reference/networks.py:364-390
 * and, below it, for what the reference reaches through kaolin (NVIDIAGameWorks/kaolin v0.12.0, not vendored):
 *     kaolin.render.mesh.prepare_vertices / dibr_rasterization / texture_mapping / spherical_harmonic_lighting
 *     (call sites networks.py:284-306) -> kaolin._C.render.mesh.{packed_rasterize_forward_cuda,
 *     rasterize_backward_cuda, dibr_soft_mask_forward_cuda, dibr_soft_mask_backward_cuda},
 *     kaolin.metrics.render.mask_iou (call site networks.py:377).
 *
 * Rules of the ABI
 *   - plain C: raw DEVICE pointers, sizes and scalars only; no torch / C++ types.
 *   - every function returns MM_OK (0) or a negative MMStatus; nothing throws across the boundary.
 *   - the library never allocates: the caller owns every buffer including the workspace
 *     (size from mm_query_workspace / mm_recon_query_workspace) and keeps the render workspace alive, unmodified,
 *     between mm_render_forward and the matching mm_render_backward.
 *   - all work is enqueued on the given HIP stream (pass the hipStream_t as a void*; NULL = the null stream);
 *     no host synchronisation, no global state, re-entrant.
 *   - all floating point is fp32; indices are int32.  Tensors are dense row-major unless strides are given.
 */
#ifndef MM_RENDER_H
#define MM_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mm_stream_t; /* hipStream_t */

typedef enum MMStatus {
    MM_OK = 0,
    MM_ERR_NULL_POINTER = -1,   /* a required pointer is NULL */
    MM_ERR_BAD_SHAPE = -2,      /* a size is <= 0 or inconsistent */
    MM_ERR_WORKSPACE = -3,      /* workspace missing or smaller than mm_query_workspace() */
    MM_ERR_LAUNCH = -4,         /* hipLaunchKernel / hipMemsetAsync reported an error */
    MM_ERR_UNSUPPORTED = -5     /* outside what the kernels implement (knum <= 0, image side > 65535, > MM_DIBR_MAX_D channels) */
} MMStatus;

/* --------------------------------------------------------------------------------------------------------------------
 * Render: replaces DiffRender.render (networks.py:258-324), i.e. camera (smr_utils.py:257-311) -> prepare_vertices ->
 * dibr_rasterization -> texture_mapping -> spherical_harmonic_lighting -> composite -> clamp -> cat(soft mask).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct MMRenderDesc {
    /* sizes */
    int32_t B, H, W;            /* batch, image rows (= round(ratio*image_size)), image cols (= image_size) */
    int32_t V, F;               /* template vertices / faces */
    int32_t Ht, Wt;             /* texture rows / cols */
    int32_t no_mask;            /* 1: composite over bg then shade (trainer's --bg); 0: white background  (:307-313) */
    int32_t knum;               /* dibr_rasterization knum (30) */
    /* constants: cam_proj (networks.py:172-174) and the dibr_rasterization defaults */
    float proj[3];              /* [1/(ratio'*tan(fovy/2)), 1/tan(fovy/2), -1] */
    float sigmainv, boxlen, multiplier, eps; /* 7000, 0.02, 1000, 1e-8 */
    /* static template data (device) */
    const int32_t* faces;       /* (F,3) vertex ids */
    const float* face_uvs;      /* (F,3,2) raw OBJ uv of every corner (networks.py:196-202) */
    const int32_t* vc_table;    /* (V,vc_stride,4) vertex -> incident corners, fixed stride (mm_build_vertex_corner_table): entry = {face*3 + corner,
                                 * the face's three vertex ids}, ascending, padded with {-1,..}   (backward only; may be NULL forward) */
    int32_t vc_stride;          /* entries per vertex (>= the largest valence of the template) */
    /* per-sample attributes (device), the 'attributes' dict of networks.py:259-270 */
    const float* vertices;      /* (B,V,3) */
    const float* textures;      /* (B,3,Ht,Wt) */
    const float* lights;        /* (B,9) */
    const float* bg;            /* (B,3,H,W); required iff no_mask */
    const float* azimuths;      /* (B) degrees */
    const float* elevations;    /* (B) degrees */
    const float* distances;     /* (B) */
    const float* biases;        /* (B,2) */
    /* outputs (device) */
    float* rgba;                /* (B,H,W,4): NHWC storage; the reference returns the (B,4,H,W) permute VIEW of it (:317).
                                 * Written by mm_render_forward; NOT read by mm_render_backward (may be NULL there, fused or not) */
    int32_t* face_idx;          /* (B,H,W): winning face per pixel, -1 = none (kaolin returns int64; int32 here) */
    float* face_normals;        /* (B,F,3): unit face normals in camera space = attributes['face_normals'] (:319) */
    float* imnormal;            /* (B,H,W,3) or NULL: attributes['imnormal'] (:320, "visualize only") */
    /* scratch */
    void* workspace;            /* >= mm_query_workspace(desc) bytes, 256-byte aligned */
    size_t workspace_bytes;
    /* optional profiling: NULL, or an array of 2*MM_PROF_RENDER_SLOTS hipEvent_t created by the caller; the library
     * records events [2*slot] / [2*slot+1] on the stream immediately before / after the kernel of that slot. */
    void** prof_events;
    /* optional FUSED reconstruction loss = DiffRender.recon_data (networks.py:364-390; its contour term: fused_contour below) folded into the render
     * kernels: with fused_gt set, mm_render_forward also reduces the loss terms while it shades, and mm_render_backward
     * derives dL/d rgba on the fly from fused_gt and the prediction it re-forms per pixel, bit for bit (`rgba` is not read back: the caller
     * may already have overwritten it; MMRenderGrads.grad_rgba is then ignored and may be NULL) and writes the loss value.
     * Same arithmetic as mm_recon_data_forward/backward; saves three launches and the grad_rgba round trip. */
    const float* fused_gt;          /* (B,4,H,W) dense rgb + mask, or NULL */
    float fused_image_weight;       /* DiffRender.image_weight */
    float* fused_loss;              /* (1) device scalar, written by mm_render_backward; may be NULL */
    const float* fused_grad_loss;   /* (1) device scalar dL/dloss, or NULL for 1 */
    int32_t options;                /* bit set of MM_OPT_* (below); 0 = the semantics of SURVEY.md 8(a) */
    /* 1: GEOMETRY ONLY -- the call site that discards the image and keeps attributes['face_normals'] (trainer.py:367:
     * `_, Aire = diffRender.render(**Aire)`).  mm_render_forward then runs the vertex stage alone (camera, prepare_vertices,
     * face_normals; nothing is rasterised, rgba / face_idx / imnormal are not written and may be NULL); mm_render_backward takes
     * MMRenderGrads.grad_face_normals (required) and writes grad_vertices and the four camera gradients only -- the texture, light and
     * background gradients of such a render are identically zero and are NOT written (their pointers may be NULL). */
    int32_t geometry_only;
    /* optional, may be NULL: one int32 the device can write -- device memory, or PINNED HOST memory, which the host can then poll without
     * synchronising.  mm_render_backward adds to it the number of texture-gradient records it had to drop (see mm_query_workspace /
     * mm_render_status): 0 stays 0.  Lets a caller that never synchronises (autograd nodes, captured graphs) still turn an overflowing
     * record pool into an error one step later instead of training on NaN texture gradients. */
    int32_t* status_flag;
    /* the fused loss's contour weight (recon_data's `contour` argument, networks.py:379-388; trainer.py:441 passes opt.lambda_contour): 0 = no
     * contour term.  > 0 needs H % 4 == 0 and W % 4 == 0 (then F.interpolate's two nearest resamplings pick the top-left pixel of every
     * 4x4 block, which lies in the pixel's own 8x8 screen tile; other sizes: MM_ERR_BAD_SHAPE -- use mm_recon_data_* for those).  Ignored
     * without fused_gt. */
    float fused_contour;
    /* DEFERRED fusion, mm_render_backward only (ABI 6): the un-modified trainer's order of calls -- `render`, then `recon_data(pred, gt)` on the image
     * that render wrote (trainer.py:276,441) -- with the fused backward.  The loss VALUE was formed by mm_recon_data_forward on the image (its own
     * launches, its own bits); fused_totals = that call's per-image totals, mm_recon_data_totals(recon desc): (B,4) floats in ITS workspace, which the
     * caller keeps alive until this backward has run.  With fused_gt AND fused_totals set, mm_render_backward forms dL/d rgba per pixel with
     * mm_recon_data_backward's own expressions from those totals and the prediction it re-forms -- bit for bit the gradient mm_recon_data_backward
     * would have written -- without that launch and without the grad_rgba round trip.  MMRenderGrads.grad_rgba, if not NULL, is ADDED to it (the
     * image's other consumers).  fused_contour must be 0 (the contour term's gradient is formed in another order by the fused kernels: use
     * mm_recon_data_backward for it); fused_loss is not written; the forward of this render ran WITHOUT fused_gt.  NULL: off. */
    const float* fused_totals;
    /* STEP MODE of the fused loss (NULL: off): the gradients of the step, named already for the FORWARD.  Where dL/dloss is known before the
     * render (a training step's loss_scale: not an autograd graph, whose dL/dloss arrives later), the pixel pass of the backward depends on
     * nothing the forward's shade epilogue does not hold in registers, so mm_render_forward runs it there and mm_render_backward launches only
     * the gathers and the vertex backward -- one kernel and one pass over the pixels less per step.
     * Contract: the field is set, to the same MMRenderGrads, for BOTH calls of a step.  mm_render_forward reads it for grad_bg (written there
     * under no_mask) and reads *fused_grad_loss, which must hold its value by then; mm_render_backward is given the same MMRenderGrads.  What the
     * forward leaves is read, not consumed: mm_render_backward may be called again after one forward.
     * Taken only with fused_gt set, fused_contour == 0, no fused_totals, no geometry_only, one view, and a shape the step kernel covers (the
     * 256-thread per-batch walk over a tile order: 8-pixel screen bins, a batch below the one-tile-per-workgroup threshold, no
     * MM_OPT_MANY_IN_FLIGHT, no forced walk form); in every other case the forward ignores the field and the backward is the usual one, with the
     * usual bits.  mm_query_workspace accounts for the step arrays when the field is set, whether the shape takes step mode or not. */
    const struct MMRenderGrads* step_grads;
} MMRenderDesc;

/* MMRenderDesc.options / MMDibrDesc.options: 0 = the semantics of SURVEY.md 8(a) (the oracle's defaults).  The bits switch,
 * one by one, the choices that SURVEY.md Appendix C lists as recalled from kaolin's sources and not re-verifiable here
 * (kaolin is not vendored): a maintainer with a CUDA box and real kaolin can pin the path by flipping a bit instead of
 * editing kernels.  oracle/mm_oracle.inc takes the same bits, and tests/ hold HIP == oracle for every one of them. */
enum { MM_OPT_WALK_BLOCK = 1 << 1,         /* tuning: force the 256-thread / cooperative-heavy-tile shape of the walk kernels ...          */
       MM_OPT_WALK_WAVE = 1 << 2,          /* ... or the one-wave-per-tile shape (default: chosen by screen-bin size and batch).  Identical forward outputs;
                                            * identical gradients too, except that with screen bins larger than a tile the 256-thread shape sweeps a few
                                            * more faces over their inflated boxes: the same integer sums cut into other items, <= 1e-9 of a gradient's maximum */
       MM_OPT_CULL_STRICT = 1 << 4,        /* rasterise faces with face_normals_z > 0 instead of >= 0                    (App. C-1) */
       MM_OPT_SOFT_SKIP_CULLED = 1 << 5,   /* the soft mask skips the faces the colour pass culls                          (App. C-1) */
       MM_OPT_BBOX_HALF_OPEN = 1 << 6,     /* a pixel centre exactly on a face's bbox edge is outside (<= / >= reject)     (App. C-4) */
       MM_OPT_BARY_ONE_MINUS = 1 << 7,     /* barycentrics as w1 = k1/(S+eps), w2 = k2/(S+eps), w0 = 1 - w1 - w2 (eps added, not
                                            * copysign'd) instead of three edge functions / copysign-padded sum          (App. C-3) */
       MM_OPT_SH_ORDER_XYZ = 1 << 8,       /* SH linear bands in x,y,z order and quadratic bands xy,yz,3z^2-1,xz,x^2-y^2 paired with
                                            * lights 1..8 in THAT order (instead of x,z,y / xy,yz,z^2,xz,x^2-y^2)          (App. C-6) */
       MM_OPT_WALK_QUEUE = 1 << 10,        /* tuning: force the compacting-queue form of the forward walk (default: screen bins larger than a tile) ...           */
       MM_OPT_WALK_BATCH = 1 << 11,        /* ... or the per-batch form (default: 8-pixel bins); identical results                                              */
       MM_OPT_MANY_IN_FLIGHT = 1 << 12,    /* hint, identical results: the caller keeps several independent calls in flight (several streams), so every launch
                                            * shares the chip -- the kernels take the shapes large batches take on their own (forward walk: one tile per
                                            * workgroup for 8-pixel screen bins; face sweep of the backward: four lanes per item).  Four B=48 steps on four
                                            * streams: +3 % images/s; ONE step at a time: -14 % (profiles/r06_many_in_flight_ab.md)                       */
       MM_OPT_ORDER_LAUNCH = 1 << 13,      /* tuning / tests, identical results: sort the tiles in a launch of their own behind the vertex stage, from the bin
                                            * masks, also where the vertex launch would sort them itself from recomputed boxes (small screens and meshes,
                                            * one view: profiles/order_beside_vertex_ab.md).  No influence on whether a call takes step mode                */
       MM_OPT_BBOX_MIN_CLOSED_MAX_OPEN = 1 << 9 };  /* bbox test [min, max): reject x < min || x >= max -- the third form upstream may have,
                                            * between the closed default and MM_OPT_BBOX_HALF_OPEN (which opens both borders)  (App. C-4) */

enum { MM_PROF_VERTEX_FWD = 0, MM_PROF_RASTER_FWD = 1, MM_PROF_PIXEL_BWD = 2, MM_PROF_GATHER_BWD = 3, MM_PROF_VERTEX_BWD = 4,
       MM_PROF_ORDER = 5, MM_PROF_RENDER_SLOTS = 6 };
enum { MM_PROF_RECON_PARTIAL = 0, MM_PROF_RECON_FINAL = 1, MM_PROF_RECON_BWD = 2, MM_PROF_RECON_CONTOUR = 3,
       MM_PROF_RECON_SLOTS = 4 };

/* Gradients of one render call.  Every non-NULL output is OVERWRITTEN (the library zero-fills what it accumulates). */
typedef struct MMRenderGrads {
    const float* grad_rgba;          /* (B,H,W,4) NHWC, dL/d rgba; required unless MMRenderDesc.fused_gt is set */
    const float* grad_face_normals;  /* (B,F,3) or NULL: dL/d attributes['face_normals'] (used by calc_reg_loss, :422-431) */
    float* grad_vertices;            /* (B,V,3) */
    float* grad_textures;            /* (B,3,Ht,Wt) */
    float* grad_lights;              /* (B,9) */
    float* grad_bg;                  /* (B,3,H,W); required iff no_mask */
    float* grad_azimuths;            /* (B) per degree */
    float* grad_elevations;          /* (B) per degree */
    float* grad_distances;           /* (B) */
    float* grad_biases;              /* (B,2) */
} MMRenderGrads;

/* The MINIMUM workspace for the shape.  Everything in it is sized for the worst case except the pool of texture-gradient records
 * (one per covered pixel and texture tile under its bilinear footprint), which holds 9/8 records per pixel: a fully covered image
 * with one footprint in eight across a tile border.  A workspace_bytes above the minimum is used: the excess enlarges the images'
 * record arrays (24 bytes per record and image).  An image that still runs out (texture coordinates that put most pixels on the
 * corners of 32x32-texel tiles) gets NaN in ALL of its grad_textures texels -- never a silently short sum -- and mm_render_status
 * says how many records were dropped. */
size_t mm_query_workspace(const MMRenderDesc* desc);
int mm_render_forward(const MMRenderDesc* desc, mm_stream_t stream);
int mm_render_backward(const MMRenderDesc* desc, const MMRenderGrads* grads, mm_stream_t stream);
/* After mm_render_backward and before the next mm_render_forward on the same workspace: copies the per-image counts of dropped
 * texture-gradient records to dropped_host (B ints, may be NULL) and returns MM_OK if all are zero, MM_ERR_WORKSPACE otherwise
 * (a NULL desc / workspace: MM_ERR_NULL_POINTER; a bad shape, a workspace below the minimum or misaligned: MM_ERR_BAD_SHAPE).
 * The one entry point that SYNCHRONISES the stream (a diagnostic, not part of a step). */
int mm_render_status(const MMRenderDesc* desc, mm_stream_t stream, int32_t* dropped_host);
/* Fused mode only (desc->fused_gt and desc->fused_loss set), after mm_render_forward: writes the recon_data value of the batch
 * (networks.py:364-390, contour = 0) to desc->fused_loss from the sums the forward left in the workspace -- for callers that need
 * the loss before they run the backward (the autograd API DiffRender.render_recon).  mm_render_backward writes the same value. */
int mm_render_fused_loss(const MMRenderDesc* desc, mm_stream_t stream);
/* 1 if mm_render_forward / mm_render_backward take STEP MODE for this descriptor (MMRenderDesc.step_grads set and every condition listed there
 * met), 0 if they ignore the field.  Looks at sizes, options and which pointers are set only; nothing is launched. */
int mm_render_step_mode(const MMRenderDesc* desc);
/* tests: byte offsets, in a workspace of this descriptor, of the tile order's per-image counts {cooperatively walked tiles, non-empty tiles, -, -}
 * (B,4) int32 [0], of the step arrays' light rows [1] and run list [2], and the run list's length per image [3] */
int mm_debug_step_layout(const MMRenderDesc* desc, size_t* out4);
/* Tools only (profiles/tools): byte offsets inside the render workspace of out[0] = chunkmap (B,F) int2, out[1] = sweep items (B,item_cap)
 * int2, out[2] = nitems (B) int2, out[3] = per-item partial sums (B,item_cap,12) float; out[4] = item_cap; out[5] = gp (B,H,W,2) float4,
 * out[6] = gp2 (B,H,W) float, out[7] = soft (B,H,W) float2, out[8] = per-texture-tile record counts of the last backward (B,ntiles) int
 * followed by the list offsets + 1 (B,ntiles) and the records dropped (B); out[9] = ntiles; out[10] = records an image's array holds;
 * out[11] = the forward's per-tile footprint counts (B,ntiles) int.  `out` has room for 16 values.  Returns 0, or MM_ERR_*. */
int mm_debug_workspace_layout(const MMRenderDesc* desc, size_t* out8);

/* --------------------------------------------------------------------------------------------------------------------
 * Multi-view render: B samples x N views in ONE pass of the render kernels over B*N images, every sample's mesh, texture, lights and
 * background read from the sample's single copy.  The reference renders the same sample under several cameras wherever it deep_copies an
 * attribute set and edits the camera (trainer.py:280-289,347 Ae / Ae90; :710-723 the five evaluation renders; :619-671 the turntables); with
 * mm_render_forward that costs a replicated copy of every per-sample tensor per view.
 *   render   an MMRenderDesc of the B*N IMAGES (render.B = B*N; image i = b*N + n, sample-major): the four camera inputs and every output are
 *            per image, exactly as in mm_render_forward -- but `vertices`, `textures`, `lights` and `bg` address (B,...) tensors, one row per
 *            SAMPLE, and image i reads row i / views.  fused_gt, fused_totals and geometry_only must be unset (MM_ERR_UNSUPPORTED).
 *   views    N >= 1; render.B must be a multiple of it (MM_ERR_BAD_SHAPE otherwise).
 * Forward: every image is bit-identical to image i of mm_render_forward on the (B*N,...) tensors replicated with repeat_interleave(N): the same
 * kernels in the shapes a batch of B*N images takes, the same workspace layout, the same texture-record pool, status word and NaN rule per image.
 * Backward: MMRenderGrads with grad_rgba, grad_face_normals and the four camera gradients per IMAGE (bit-identical to mm_render_backward's) and
 * grad_vertices, grad_textures, grad_lights, grad_bg shaped (B,...): for each the kernels write the per-image gradients mm_render_backward would
 * have written into a staging area of the workspace, and one more launch adds a sample's views up in ascending view order,
 * ((g0 + g1) + g2) + ..., plain fp32 adds (no fma, no atomics): bitwise reproducible.  With views == 1 nothing is staged and nothing more is
 * launched: the two calls are mm_render_forward / mm_render_backward.
 * Workspace: mm_render_views_query_workspace = mm_query_workspace(&render) for views == 1, else that plus the four staging areas (each
 * B*N rows, rounded up to 256 bytes; bg's too when no_mask is 0, so that the size depends on the shape alone).  Both calls take the SAME
 * workspace and workspace_bytes; the staging areas come first, the render workspace of the B*N images takes all the rest (what exceeds the
 * query enlarges the record arrays as in mm_render_forward).  mm_render_status is asked with a copy of `render` whose workspace is that
 * rest: workspace + (query - mm_query_workspace(&render)), workspace_bytes less the same.  B <= 65535 samples.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct MMRenderViewsDesc {
    MMRenderDesc render;
    int32_t views;
} MMRenderViewsDesc;

size_t mm_render_views_query_workspace(const MMRenderViewsDesc* desc);
int mm_render_views_forward(const MMRenderViewsDesc* desc, mm_stream_t stream);
int mm_render_views_backward(const MMRenderViewsDesc* desc, const MMRenderGrads* grads, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Indexed render: M images in ONE pass of the render kernels, each of which picks its mesh, its texture, its lights and its background
 * by a row index of its own.  The multi-view render above is the pattern "image i reads row i / N"; the reference renders a second one
 * as often -- every texture on every shape (show_rainbow2.py:376-399), every deep_copy(Ae, index=...) followed by a render
 * (networks.py:146-161, trainer.py:293-308), texture rows picked out of a pool with a row count of its own
 * (generate_market_new_class9.py:331-336) -- and with mm_render_forward each costs a gathered copy of every tensor.
 *   render   an MMRenderDesc of the M IMAGES (render.B = M): the four camera inputs and every output are per image, exactly as in
 *            mm_render_forward; `vertices`, `textures`, `lights` and `bg` address tensors of rows[0..3] rows.  fused_gt, fused_totals and
 *            geometry_only must be unset (MM_ERR_UNSUPPORTED); step_grads is ignored.
 *   rows     {R_v, R_t, R_l, R_bg}, each >= 1 (R_bg is looked at under no_mask only).
 *   index    per tensor (M) int32 in device memory: image i reads row index[t][i].  NULL: the identity, and rows[t] must equal M.
 *   backward 0: a forward-only call -- the workspace holds no staging and mm_render_indexed_backward refuses it (MM_ERR_WORKSPACE).
 *   status_flag  optional; device or pinned host memory.  The forward ADDS the number of index entries outside [0, rows[t]) to it.
 * The forward's first launch turns the index tensors into a plan in the workspace's head (no host synchronisation, nothing read back):
 * per tensor a sanitised table -- the only table a later kernel reads; an out-of-range entry becomes 0, is counted into the status
 * word and marks its IMAGE bad -- and, for the backward, the rows' image lists (offsets, images in ascending image order, bad images left
 * out).  A bad image gets rgba = NaN in all four channels and face_idx = -1; nothing is read through its raw index.
 * Forward: a good image is bit-identical to image i of mm_render_forward on the tensors gathered with index_select.
 * Backward: grad_rgba, grad_face_normals and the four camera gradients per IMAGE (bit-identical to mm_render_backward's; NaN for a bad
 * image); grad_vertices, grad_textures, grad_lights, grad_bg shaped like the inputs, (rows[t],...): the kernels write the per-image
 * gradients into staging areas of the workspace and one last launch adds up each row's list in ascending image order,
 * ((g[i0] + g[i1]) + g[i2]) + ..., plain fp32 adds (no fma, no atomics): bitwise reproducible.  A row no image reads gets zeros.
 * Workspace: the head -- the plan, and with `backward` the four staging areas of M rows each, as in the multi-view call -- then the render
 * workspace of the M images with all the bytes that are left.  mm_render_status is asked with a copy of `render` whose workspace starts
 * query - mm_query_workspace(&render) bytes in.  M <= 65535 and every rows[t] <= 65535 (MM_ERR_UNSUPPORTED; the query returns 0).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct MMRenderIndexedDesc {
    MMRenderDesc render;
    int32_t rows[4];
    const int32_t* index[4];
    int32_t backward;
    int32_t* status_flag;
} MMRenderIndexedDesc;

size_t mm_render_indexed_query_workspace(const MMRenderIndexedDesc* desc);
int mm_render_indexed_forward(const MMRenderIndexedDesc* desc, mm_stream_t stream);
int mm_render_indexed_backward(const MMRenderIndexedDesc* desc, const MMRenderGrads* grads, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Reconstruction loss: replaces DiffRender.recon_data (networks.py:364-390) incl. kaolin mask_iou (:377) and the
 * optional contour term (:379-387):  loss = image_weight * mean|pred*gm+(1-gm) - (gt*gm+(1-gm))| + (1 - mean_b IoU_b)
 *                                           [+ contour * mean((c(pred_mask) - c(gt_mask))^2)].
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct MMReconDesc {
    int32_t B, H, W;
    const float* pred;           /* rgba prediction, element strides below (NHWC storage from mm_render_forward: {4HW,1,4W,4}) */
    int64_t pred_strides[4];     /* strides of (b, channel, y, x) in elements */
    const float* gt;             /* (B,4,H,W) dense: rgb + binary mask */
    float image_weight;          /* DiffRender.image_weight */
    float contour;               /* lambda_contour; <= 0 disables the term */
    float* loss;                 /* (1) device scalar, overwritten */
    /* backward only */
    const float* grad_loss;      /* (1) device scalar dL/dloss, or NULL for 1 */
    float* grad_pred;            /* same strides as pred; overwritten */
    void* workspace;             /* >= mm_recon_query_workspace(desc) bytes; forward fills it, backward reads it */
    size_t workspace_bytes;
    void** prof_events;          /* optional: 2*MM_PROF_RECON_SLOTS hipEvent_t, as in MMRenderDesc */
} MMReconDesc;

size_t mm_recon_query_workspace(const MMReconDesc* desc);
int mm_recon_data_forward(const MMReconDesc* desc, mm_stream_t stream);
int mm_recon_data_backward(const MMReconDesc* desc, mm_stream_t stream);
/* Where mm_recon_data_forward left the per-image totals {sum|pi-gi|, sum p*g, sum p+g-p*g, contour sum} (B,4) inside desc->workspace: what
 * MMRenderDesc.fused_totals takes (deferred fusion).  NULL if desc or its workspace is NULL / too small. */
const float* mm_recon_data_totals(const MMReconDesc* desc);

/* --------------------------------------------------------------------------------------------------------------------
 * Nearest neighbour of every point of x (B,N,3) in y (B,M,3): squared distance (B,N) and index (B,N) int32, lowest index
 * on ties; NaN distances never win, and a query with no finite distance gets index 0 and distance +inf.  B <= 65535.  The
 * O(N*M) half of pytorch3d.loss.chamfer_distance (knn_points, K=1) that DiffRender.recon_att(chamfer=True) needs
 * (networks.py:342,356); the differentiable tail is mm_chamfer_backward below.
 * ------------------------------------------------------------------------------------------------------------------ */
int mm_nearest_neighbour(int32_t B, int32_t N, int32_t M, const float* x, const float* y, float* dist, int32_t* idx,
                         mm_stream_t stream);
/* Both directions of pytorch3d.loss.chamfer_distance in ONE launch (networks.py:342,356 always needs both): for every x its
 * nearest y (dist_x, idx_x: (B,N)) and for every y its nearest x (dist_y, idx_y: (B,M)).  Same results as two calls above. */
int mm_chamfer_nearest(int32_t B, int32_t N, int32_t M, const float* x, const float* y, float* dist_x, int32_t* idx_x,
                       float* dist_y, int32_t* idx_y, mm_stream_t stream);
/* Gradient of the chamfer loss  L = mean_b [ mean_i |x_i - y_{idx_x,i}|^2 + mean_j |y_j - x_{idx_y,j}|^2 ]  with the indices
 * mm_chamfer_nearest wrote (in range: [0,M) and [0,N)):
 *   grad_x_i = wx (x_i - y_{idx_x,i}) - wy sum_{j : idx_y,j = i} (y_j - x_i),   grad_y_j = wy (y_j - x_{idx_y,j}) - wx sum_{i : idx_x,i = j} (x_i - y_j),
 * wx = 2g / (B N), wy = 2g / (B M), g = *grad_loss (one float in device memory, read by the kernel).  grad_x (B,N,3), grad_y (B,M,3)
 * are overwritten.  Every sum is taken in ascending source index, without atomics: bitwise reproducible, and a batch row's result
 * does not depend on the other rows.  Like the two searches above: B <= 65535 (MM_ERR_UNSUPPORTED otherwise). */
int mm_chamfer_backward(int32_t B, int32_t N, int32_t M, const float* x, const float* y, const int32_t* idx_x, const int32_t* idx_y,
                        const float* grad_loss, float* grad_x, float* grad_y, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Mesh regularisers: replaces DiffRender.calc_reg_loss / calc_reg_edge / calc_reg_depth /
 * calc_reg_depthR / calc_reg_depthC / calc_reg_deform / recon_flip(L1=False) (networks.py:392-491; orchestrated by
 * trainer.py:54-74), one launch per direction for any subset of the terms.  losses[k] is the reference's value of term k
 * (calc_reg_loss = lambda_lpl * losses[LAPLACIAN] + lambda_flat * losses[FLAT]; calc_reg_edge = losses[EDGE], which already
 * carries the reference's 0.1); terms that were not requested read 0.
 * ------------------------------------------------------------------------------------------------------------------ */
enum { MM_REG_LAPLACIAN = 0, MM_REG_FLAT = 1, MM_REG_EDGE = 2, MM_REG_DEPTH = 3, MM_REG_DEPTHR = 4, MM_REG_DEPTHC = 5,
       MM_REG_DEFORM = 6, MM_REG_FLIP = 7, MM_REG_TERMS = 8 };

typedef struct MMMeshRegDesc {
    int32_t B, V, F, E;         /* batch, template vertices / faces / unique edges */
    uint32_t terms;             /* bit k set: compute term k */
    /* static template tables (device).  The (V,V) laplacian (networks.py:249) and its transpose as CSR, diagonal included */
    const int32_t* lap_offsets;   const int32_t* lap_cols;   const float* lap_vals;
    const int32_t* lapT_offsets;  const int32_t* lapT_cols;  const float* lapT_vals;    /* backward only */
    const int32_t* edges;         /* (E,2)  vertex ids                                   (:220-233) */
    const int32_t* edge2faces;    /* (E,2)  the two faces of every edge                  (:235-246) */
    const int32_t* ve_offsets;    const int32_t* ve_items;   /* vertex -> edge*2 + end   (backward only) */
    const int32_t* fe_offsets;    const int32_t* fe_items;   /* face   -> edge*2 + side  (backward only) */
    const int32_t* flip_index;    /* (V)    mirrored partner of every vertex             (:215-217) */
    const int32_t* flipT_offsets; const int32_t* flipT_items; /* u -> {v : flip_index[v] == u}  (backward only) */
    const float* sign_init;       /* (V)    sign of the template's z                     (:213) */
    /* inputs (device); one may be NULL if no requested term reads it */
    const float* vertices;        /* (B,V,3)  EDGE, DEPTH, DEPTHR, DEPTHC */
    const float* delta_vertices;  /* (B,V,3)  LAPLACIAN, DEFORM, FLIP */
    const float* face_normals;    /* (B,F,3)  FLAT */
    float ratio, temp, eps;       /* DiffRender.ratio; calc_reg_depthR's temp (2); depthR / depthC eps (0.001) */
    float* losses;                /* (MM_REG_TERMS) device */
    void* workspace;              /* >= mm_mesh_reg_query_workspace bytes, 256-byte aligned, ZERO-FILLED by the caller before its
                                   * first use; the library leaves it ready for the next call.  The backward reads what the
                                   * forward of the same inputs left in it. */
    size_t workspace_bytes;
} MMMeshRegDesc;

typedef struct MMMeshRegGrads {
    const float* weights;         /* (MM_REG_TERMS) device: dL/d losses[k] */
    float* grad_vertices;         /* (B,V,3) or NULL; overwritten */
    float* grad_delta_vertices;   /* (B,V,3) or NULL; overwritten */
    float* grad_face_normals;     /* (B,F,3) or NULL; overwritten */
} MMMeshRegGrads;

size_t mm_mesh_reg_query_workspace(const MMMeshRegDesc* desc);
int mm_mesh_reg_forward(const MMMeshRegDesc* desc, mm_stream_t stream);
int mm_mesh_reg_backward(const MMMeshRegDesc* desc, const MMMeshRegGrads* grads, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Attribute-reconstruction losses: replaces the seven means of DiffRender.recon_att
 * (networks.py:326-362; the chamfer variant of the shape term goes through mm_nearest_neighbour instead).
 * losses = { azim, elev, dist, bias, shape, texture, light }: mean |a-b| (l1 = 1) or mean (a-b)^2 (l1 = 0) over all
 * elements, azimuths / elevations through angle2xy (cos, sin of the angle in degrees).  The reference composes
 * loss_cam = azim * losses[0] + losses[1] + losses[2], loss_light = 0.1 * losses[6].
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct MMAttributes {     /* device pointers; in MMAttLossGrads any may be NULL (= that gradient is not wanted) */
    float* azimuths;              /* (B) degrees */
    float* elevations;            /* (B) degrees */
    float* distances;             /* (B) */
    float* biases;                /* (B,2) */
    float* vertices;              /* (B,V,3) */
    float* textures;              /* (B,3,Ht,Wt) */
    float* lights;                /* (B,9) */
} MMAttributes;

typedef struct MMAttLossDesc {
    int32_t B, V, Ht, Wt;
    int32_t l1;                   /* 1: mean |a-b| (opt.L1), 0: mean (a-b)^2 */
    MMAttributes pred, target;    /* read only; all seven required */
    float* losses;                /* (7) device */
    void* workspace;              /* >= mm_attribute_loss_query_workspace bytes, 256-byte aligned, ZERO-FILLED before its first use */
    size_t workspace_bytes;
} MMAttLossDesc;

typedef struct MMAttLossGrads {
    const float* weights;         /* (7) device: dL/d losses[k] */
    MMAttributes pred, target;    /* outputs, overwritten; NULL members are skipped */
} MMAttLossGrads;

size_t mm_attribute_loss_query_workspace(const MMAttLossDesc* desc);
int mm_attribute_loss_forward(const MMAttLossDesc* desc, mm_stream_t stream);
int mm_attribute_loss_backward(const MMAttLossDesc* desc, const MMAttLossGrads* grads, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Disentangle regularisation of the generator step (--dis1 / --dis2, trainer.py:455-494).
 *
 * mm_disentangle_inputs: the two extra encoder batches in one launch, both NCHW-contiguous and pure copies --
 *   out_flip[b,c,y,x]  = x[b,c,y,W-1-x]                                   (fliplr(Xa))
 *   out_erase[b,c,y,x] = value inside the sample's box, x[b,c,y,x] outside  (RandomErasing(p=1)(Xa), all C channels)
 * A box is (i, j, h, w): rows [i, i+h), columns [j, j+w), clamped to the image on the device; h or w < 1 erases nothing.
 * `boxes` NULL: `box` serves the whole batch (the reference's form).  Otherwise a (B,4) int32 DEVICE array, one box per
 * sample, read by the kernel without a synchronisation; boxes_rows states how many rows it has and must be B.
 * Rows are walked in 16-byte pieces where W % 4 == 0 and x and the outputs are 16-byte aligned (NHWC: C = 3 or 4 too);
 * otherwise one element at a time.  B*C*H*W must fit an int32 (MM_ERR_UNSUPPORTED).
 *
 * mm_disentangle_forward: terms = { l_text, l_shape_flip, l_azim, l_elev, l_dist, l_bias, l_shape_jitter } with
 *   l_text         mean over B*3*Ht*Wt of |Tf[b,c,y,Wt-1-x] - T[b,c,y,x]|         (Tf is read mirrored; nothing is copied)
 *   l_shape_flip   mean over b of sqrt(sum_{v,k} (Vf[b,v,k] - s_k V[b,v,k])^2), s = (-1, 1, 1)
 *   l_azim, l_elev mean over B*2 of the squared differences of (cos, sin) of the angles in degrees (angle2xy)
 *   l_dist, l_bias mean over B and B*2 of the squared differences
 *   l_shape_jitter mean over b of sqrt(sum (dVj[b] - dV[b])^2) on delta_vertices
 * The flip set (flip_textures, flip_vertices: both or neither) feeds terms 0-1 and needs textures and vertices; the jitter
 * set (the five jitter_* pointers: all or none) feeds terms 2-6 and needs the other five.  A missing set leaves its
 * terms 0 and none of its pointers is read.  The reference composes
 *   dis1 * (terms[0] + terms[1]) + dis2 * ((azim * terms[2] + terms[3] + terms[4] + terms[5]) + terms[6]).
 * Sums: every workgroup adds its texels in a fixed order, per-sample sums of squares are one workgroup's block sum, and
 * the last workgroup to finish adds the partials in a fixed order and takes the square roots -- no float atomics, the
 * same bits run to run.  The (B,2) norms stay in the workspace for the backward, which therefore takes the workspace of
 * its forward.  B*3*Ht*Wt must fit an int32 (MM_ERR_UNSUPPORTED).
 * mm_disentangle_backward: every gradient of BOTH sets in one launch, each element written once, NULL members skipped;
 * a norm term's gradient is weights[k] / B * diff / norm, exactly 0 for a sample whose norm is 0.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct MMDisentangleInputsDesc {
    int32_t B, C, H, W;
    int32_t nhwc;                 /* 0: x is NCHW-contiguous, 1: NHWC-dense (a render) */
    int32_t box[4];               /* i, j, h, w: the one box of the batch when boxes is NULL */
    int32_t boxes_rows;           /* rows of boxes; must be B when boxes is given */
    float value;                  /* written into the box */
    const float* x;               /* (B,C,H,W) in the layout nhwc names */
    const int32_t* boxes;         /* (B,4) device, or NULL */
    float* out_flip;              /* (B,C,H,W) NCHW, or NULL */
    float* out_erase;             /* (B,C,H,W) NCHW, or NULL (at least one output is required) */
} MMDisentangleInputsDesc;

int mm_disentangle_inputs(const MMDisentangleInputsDesc* desc, mm_stream_t stream);

typedef struct MMDisentangleDesc {
    int32_t B, V, Ht, Wt;
    const float* textures;        /* (B,3,Ht,Wt)  Ae; read only, like every input below */
    const float* vertices;        /* (B,V,3) */
    const float* azimuths;        /* (B) degrees */
    const float* elevations;      /* (B) degrees */
    const float* distances;       /* (B) */
    const float* biases;          /* (B,2) */
    const float* delta_vertices;  /* (B,V,3) */
    const float* flip_textures;   /* Ae_fliplr: both or neither */
    const float* flip_vertices;
    const float* jitter_azimuths; /* Ae_jitter: all five or none */
    const float* jitter_elevations;
    const float* jitter_distances;
    const float* jitter_biases;
    const float* jitter_delta_vertices;
    float* terms;                 /* (7) device */
    void* workspace;              /* >= mm_disentangle_query_workspace bytes, 256-byte aligned, ZERO-FILLED before its first use */
    size_t workspace_bytes;
} MMDisentangleDesc;

typedef struct MMDisentangleGrads {
    const float* weights;         /* (7) device: dL/d terms[k] */
    float* textures;              /* outputs, overwritten, shaped like the inputs of the same name; NULL members are skipped */
    float* vertices;
    float* azimuths;
    float* elevations;
    float* distances;
    float* biases;
    float* delta_vertices;
    float* flip_textures;
    float* flip_vertices;
    float* jitter_azimuths;
    float* jitter_elevations;
    float* jitter_distances;
    float* jitter_biases;
    float* jitter_delta_vertices;
} MMDisentangleGrads;

size_t mm_disentangle_query_workspace(const MMDisentangleDesc* desc);
int mm_disentangle_forward(const MMDisentangleDesc* desc, mm_stream_t stream);
int mm_disentangle_backward(const MMDisentangleDesc* desc, const MMDisentangleGrads* grads, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Texture-flow sampling: the tail of TextureEncoder.forward (network/model_res.py:597-612, makeup = 0),
 * i.e. the step that produces the texture the render path consumes:
 *   textures = cat([t, t.flip(2)], 2),  t = F.grid_sample(image, flow.permute(0,2,3,1), mode='bicubic', align_corners=True)
 * (zeros padding, ATen's bicubic: A = -0.75).  flow is taken channel-first, exactly as the decoder emits it.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct MMTexFlowDesc {
    int32_t B, C, H, W;         /* image batch, channels (3), rows, cols */
    int32_t Ho, Wo;             /* flow / sampled rows, cols; the texture has 2*Ho rows */
    const float* image;         /* (B,C,H,W) */
    const float* flow;          /* (B,2,Ho,Wo): x then y, in [-1,1] */
    float* textures;            /* (B,C,2*Ho,Wo); unused by the backward */
} MMTexFlowDesc;

typedef struct MMTexFlowGrads {
    const float* grad_textures; /* (B,C,2*Ho,Wo) */
    float* grad_flow;           /* (B,2,Ho,Wo); overwritten */
    float* grad_image;          /* (B,C,H,W) or NULL; overwritten (zero-filled on the stream, then float atomics) */
} MMTexFlowGrads;

int mm_texture_flow_forward(const MMTexFlowDesc* desc, mm_stream_t stream);
int mm_texture_flow_backward(const MMTexFlowDesc* desc, const MMTexFlowGrads* grads, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Op boundary: the kaolin / pytorch3d operators the reference imports at module top (networks.py:6-19, trainer.py:31-40),
 * un-fused, one entry point per operator and direction.  The Python package 3d-magic-mirror_amd/shim exposes them under
 * kaolin's own module paths and signatures, so networks.py / trainer.py import and run unmodified.
 * They run the SAME device code as the fused render path (the same candidate walk, barycentrics, bilinear fetch and SH bands),
 * so face_idx is identical between the two boundaries.  Upstream semantics: NVIDIAGameWorks/kaolin v0.12.0 (not vendored;
 * restated in SURVEY.md 8(a)); gradients SURVEY.md Appendix A.
 * ------------------------------------------------------------------------------------------------------------------ */

/* kaolin.render.mesh.prepare_vertices(vertices, faces, camera_proj, camera_transform=...)   (call site networks.py:284-287):
 * vc = [v,1] @ T; vi = (vc.xy * proj.xy) / (vc.z * proj.z); gather by faces; unit normals with +1e-10 on the length. */
typedef struct MMPrepareDesc {
    int32_t B, V, F;
    float proj[3];                  /* camera_proj (3,1) */
    const int32_t* faces;           /* (F,3) */
    const int32_t* vc_offsets;      /* (V+1) vertex -> corner CSR (mm_build_vertex_corner_csr); backward only */
    const int32_t* vc_items;        /* (3F) */
    const float* vertices;          /* (B,V,3) */
    const float* transform;         /* (B,4,3) camera_transform [R;t] */
    float* face_vertices_camera;    /* (B,F,3,3) */
    float* face_vertices_image;     /* (B,F,3,2) */
    float* face_normals;            /* (B,F,3)   */
    void* workspace;                /* backward only: >= mm_prepare_vertices_query_workspace bytes (per-workgroup dT partials) */
    size_t workspace_bytes;
    const float* proj_device;       /* optional: camera_proj as 3 floats in DEVICE memory, read instead of proj[] -- a caller whose projection
                                     * is a device tensor (kaolin's prepare_vertices takes one) needs no device -> host read */
} MMPrepareDesc;

typedef struct MMPrepareGrads {
    const float* grad_face_vertices_camera;  /* (B,F,3,3) or NULL */
    const float* grad_face_vertices_image;   /* (B,F,3,2) or NULL */
    const float* grad_face_normals;          /* (B,F,3)   or NULL */
    float* grad_vertices;                    /* (B,V,3) overwritten */
    float* grad_transform;                   /* (B,4,3) overwritten, or NULL */
} MMPrepareGrads;

size_t mm_prepare_vertices_query_workspace(const MMPrepareDesc* desc);
int mm_prepare_vertices_forward(const MMPrepareDesc* desc, mm_stream_t stream);
int mm_prepare_vertices_backward(const MMPrepareDesc* desc, const MMPrepareGrads* grads, mm_stream_t stream);

/* kaolin.ops.mesh.face_normals(face_vertices (n,3,3), unit)   (call site networks.py:289): cross(v1-v0, v2-v0), optionally
 * divided by (length + 1e-10).  n = B*F faces.  backward: grad_normals (n,3) -> grad_face_vertices (n,3,3), overwritten. */
int mm_face_normals_forward(int64_t n, int32_t unit, const float* face_vertices, float* normals, mm_stream_t stream);
int mm_face_normals_backward(int64_t n, int32_t unit, const float* face_vertices, const float* grad_normals,
                             float* grad_face_vertices, mm_stream_t stream);

/* kaolin.render.mesh.dibr_rasterization(height, width, face_vertices_z, face_vertices_image, face_features, face_normals_z,
 * sigmainv=7000, boxlen=0.02, knum=30, multiplier=1000, eps=1e-8)   (call site networks.py:297-299)
 *   = rasterize (kaolin._C packed_rasterize_forward_cuda / rasterize_backward_cuda, K1/K2)
 *   + dibr_soft_mask (dibr_soft_mask_forward_cuda / _backward_cuda, K3/K4).
 * Outputs as kaolin returns them: interpolated features (zeros where uncovered), soft mask, int64 face_idx (-1 = none).
 * Gradients only to face_vertices_image and face_features (none to z / normals_z, like upstream). */
#define MM_DIBR_MAX_D 32            /* feature channels per corner the backward's LDS accumulators hold */
typedef struct MMDibrDesc {
    int32_t B, H, W, F, D, knum;
    float sigmainv, boxlen, multiplier, eps;
    const float* face_vertices_z;       /* (B,F,3) */
    const float* face_vertices_image;   /* (B,F,3,2) */
    const float* face_features;         /* (B,F,3,D) (a list of feature tensors is concatenated by the caller) */
    const float* face_normals_z;        /* (B,F) : faces with normal z >= 0 are rasterised */
    float* interpolated_features;       /* (B,H,W,D) */
    float* soft_mask;                   /* (B,H,W) */
    int64_t* face_idx;                  /* (B,H,W) */
    void* workspace;                    /* >= mm_dibr_query_workspace bytes, 256-byte aligned; filled by the forward, read by the backward */
    size_t workspace_bytes;
    int32_t options;                    /* MM_OPT_* bits (0 = defaults) */
} MMDibrDesc;

typedef struct MMDibrGrads {
    const float* grad_interpolated_features;   /* (B,H,W,D) or NULL */
    const float* grad_soft_mask;               /* (B,H,W)   or NULL */
    float* grad_face_vertices_image;           /* (B,F,3,2) overwritten */
    float* grad_face_features;                 /* (B,F,3,D) overwritten, or NULL */
} MMDibrGrads;

size_t mm_dibr_query_workspace(const MMDibrDesc* desc);
int mm_dibr_rasterization_forward(const MMDibrDesc* desc, mm_stream_t stream);
int mm_dibr_rasterization_backward(const MMDibrDesc* desc, const MMDibrGrads* grads, mm_stream_t stream);

/* kaolin.render.mesh.texture_mapping(texture_coordinates, texture_maps, mode)   (call site networks.py:305)
 * = F.grid_sample(maps, (2u-1, -(2v-1)), mode, align_corners=False, padding_mode='border').  N = points per batch item (H*W). */
enum { MM_TEXMAP_NEAREST = 0, MM_TEXMAP_BILINEAR = 1 };
typedef struct MMTexMapDesc {
    int32_t B, N, C, Ht, Wt, mode;
    const float* uv;                /* (B,N,2) */
    const float* textures;          /* (B,C,Ht,Wt) */
    float* out;                     /* (B,N,C) */
} MMTexMapDesc;
typedef struct MMTexMapGrads {
    const float* grad_out;          /* (B,N,C) */
    float* grad_uv;                 /* (B,N,2) overwritten, or NULL (zero for MM_TEXMAP_NEAREST) */
    float* grad_textures;           /* (B,C,Ht,Wt) overwritten, or NULL */
    /* optional scratch of >= mm_texture_mapping_backward_query_workspace bytes (256-byte aligned).  With it the texture gradient is
     * accumulated in 64-bit FIXED POINT (per-image power-of-two scale from max |grad_out|; integer adds commute) and is bitwise
     * reproducible; without it (NULL) the scatter uses float atomics (order-dependent in the last bits).
     * NON-FINITE grad_out: the two forms differ.  The fixed-point form scales by the image's max |grad_out|, so ONE NaN / inf element turns the
     * image's WHOLE texture gradient into NaN (loud, never a silently wrong finite value); the float-atomic form -- like ATen's grid_sampler and
     * kaolin -- poisons only the texels under that element's footprint.  Code that masks NaNs per texel must pass workspace = NULL. */
    void* workspace;
    size_t workspace_bytes;
} MMTexMapGrads;
size_t mm_texture_mapping_backward_query_workspace(const MMTexMapDesc* desc);
int mm_texture_mapping_forward(const MMTexMapDesc* desc, mm_stream_t stream);
int mm_texture_mapping_backward(const MMTexMapDesc* desc, const MMTexMapGrads* grads, mm_stream_t stream);

/* kaolin.render.mesh.spherical_harmonic_lighting(imnormal (B,N,3), lights (B,9)) -> (B,N)   (call site networks.py:306) */
typedef struct MMShDesc {
    int32_t B, N;
    const float* normals;           /* (B,N,3) */
    const float* lights;            /* (B,9) */
    float* out;                     /* (B,N) */
} MMShDesc;
typedef struct MMShGrads {
    const float* grad_out;          /* (B,N) */
    float* grad_normals;            /* (B,N,3) overwritten, or NULL */
    float* grad_lights;             /* (B,9) overwritten (zero-filled on the stream, one float atomic per wave and band), or NULL */
} MMShGrads;
int mm_sh_lighting_forward(const MMShDesc* desc, mm_stream_t stream);
int mm_sh_lighting_backward(const MMShDesc* desc, const MMShGrads* grads, mm_stream_t stream);

/* kaolin.metrics.render.mask_iou(lhs (B,H,W), rhs (B,H,W)) = 1 - mean_b[ sum(l*r) / (sum(l+r-l*r) + 1e-10) ]
 * (call sites networks.py:377, trainer.py:793,933).  sums: (B,2) device scratch written by the forward and read by the backward. */
typedef struct MMMaskIouDesc {
    int32_t B, N;                   /* N = H*W */
    const float* lhs; const float* rhs;
    float* sums;                    /* (B,2): {sum l*r, sum l+r-l*r} */
    float* loss;                    /* (1) */
} MMMaskIouDesc;
int mm_mask_iou_forward(const MMMaskIouDesc* desc, mm_stream_t stream);
int mm_mask_iou_backward(const MMMaskIouDesc* desc, const float* grad_loss, float* grad_lhs, float* grad_rhs, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * SSIM: pytorch_msssim._ssim, the reference's evaluation metric (trainer.py:771-795, 911-935; test.py:428-457), as one fused pass
 * per (n, c) plane.  The window is separable: the same 1-D taps along H, then along W, in *valid* mode; a dimension shorter than the
 * window is not filtered (upstream's skip rule), so Ho = H - win_size + 1 (or H), Wo likewise, P = Ho*Wo.  Per output pixel:
 *     cs_map = (2 sxy + C2) / (sx2 + sy2 + C2),  ssim_map = (2 mx my + C1) / (mx^2 + my^2 + C1) * cs_map
 * and the per-channel values are the means of both maps over the plane.  Deterministic (fixed-order reductions, no float atomics);
 * an image's values do not depend on the other images of the batch.  Two launches per call, each direction.
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_SSIM_MAX_WIN 31          /* largest win_size */
#define MM_SSIM_NONNEG 1            /* flags: relu on the per-channel ssim before mean_c / mean_all (pytorch_msssim's nonnegative_ssim) */
typedef struct MMSsimDesc {
    int32_t N, C, H, W;             /* sides <= 65535 */
    const float* x;                 /* (N,C,H,W) at x + n*x_strides[0] + c*x_strides[1] + h*x_strides[2] + w*x_strides[3] (elements) */
    int64_t x_strides[4];
    const float* y;                 /* the same for Y */
    int64_t y_strides[4];
    int32_t win_size;               /* odd, 1..MM_SSIM_MAX_WIN */
    float win[MM_SSIM_MAX_WIN];     /* the 1-D taps, first win_size used */
    float C1, C2;                   /* (K1*data_range)^2, (K2*data_range)^2 */
    int32_t flags;                  /* MM_SSIM_* */
    float* ssim;                    /* (N,C) per-channel ssim (before MM_SSIM_NONNEG), written by the forward; required */
    float* cs;                      /* (N,C) per-channel cs, or NULL */
    float* mean_c;                  /* (N) mean over C of the per-channel ssim (after MM_SSIM_NONNEG), or NULL */
    float* mean_all;                /* (1) mean over N and C (the same), or NULL */
    void* workspace;                /* mm_ssim_query_workspace bytes; scratch of either direction, nothing carried between them */
    size_t workspace_bytes;
} MMSsimDesc;
typedef struct MMSsimGrads {
    const float* grad_ssim;         /* (N,C) dL/d(per-channel ssim, before MM_SSIM_NONNEG), or NULL */
    const float* grad_cs;           /* (N,C) dL/d(per-channel cs), or NULL; not both NULL */
    float* grad_x;                  /* (N,C,H,W) dense, overwritten, or NULL */
    float* grad_y;                  /* the same for Y, or NULL; not both NULL */
} MMSsimGrads;
/* bytes of workspace for forward and backward of this shape; 0 for a bad shape */
size_t mm_ssim_query_workspace(const MMSsimDesc* desc);
/* Writes ssim (and cs, mean_c, mean_all where given).  Outputs and ssim's desc fields are ignored by the backward, which recomputes
 * the moments from x and y. */
int mm_ssim_forward(const MMSsimDesc* desc, mm_stream_t stream);
int mm_ssim_backward(const MMSsimDesc* desc, const MMSsimGrads* grads, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Template-anchored encoder features: the non-convolutional block the shape and camera encoders run on their backbone's
 * (B,C,H,W) map (reference network/model_res.py: ShapeEncoder.forward, CameraEncoder.forward).  Per (b, c) plane:
 *   local[v] = bilinear sample at template (x, y) = columns 0, 1 in [-1, 1] (-1 = first column / row), zero padding
 *   mmpool   = sigmoid(p) * max + (1 - sigmoid(p)) * mean, over an adaptive-pool bin [floor(i n / k), ceil((i + 1) n / k))
 * Shape:  out (B, 3C+3, V) = cat(local, mmpool_1x1 repeated over V, neighbor, template xyz), align_corners = 1, where
 *         neighbor[u] = sum_v local[v] lpl[v,u] over the non-zeros of the (V,V) lpl, given as two fixed-stride tables.
 * Camera: out (B, 2C, 2, 2) = cat(mmpool_2x2(x; p_map), mmpool_2x2(local as a (V,1) map; p_local)), align_corners = 0.
 * The max's gradient goes to the FIRST maximal element of a bin in row-major order.  No float atomics: every sum has a fixed
 * order, so both directions are bitwise reproducible.  The forward is one launch and needs no workspace; the backward builds
 * the per-pixel (vertex, weight) list of the bilinear taps in the workspace (three launches), applies the taps as a gather,
 * and sums the p gradients in a fixed order (two launches).
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_ENCFEAT_MAX_V 14336      /* most template vertices (one float per vertex in LDS) */
enum { MM_DTYPE_F32 = 0, MM_DTYPE_F16 = 1, MM_DTYPE_BF16 = 2 };
typedef struct MMShapeFeatDesc {
    int32_t B, C, H, W, V;          /* B*C <= 2^31 - 1, H*W <= 2^30, V <= MM_ENCFEAT_MAX_V */
    int32_t x_dtype;                /* MM_DTYPE_* */
    const void* x;                  /* (B,C,H,W) at x + b*x_strides[0] + c*x_strides[1] + h*x_strides[2] + w*x_strides[3] (elements) */
    int64_t x_strides[4];
    const float* template_xyz;      /* (V,3) dense */
    int32_t col_k;                  /* entries per column of lpl, 1..V */
    const int32_t* col_idx;         /* (col_k, V): row v of the k-th non-zero of column u at [k*V + u], -1 = none */
    const float* col_val;           /* (col_k, V): lpl[v,u] there (0 where none) */
    int32_t row_k;                  /* entries per row of lpl, 1..V */
    const int32_t* row_idx;         /* (row_k, V): column u of the k-th non-zero of row v at [k*V + v], -1 = none (backward) */
    const float* row_val;           /* (row_k, V) */
    const float* p;                 /* (1) MMPool.p, device memory */
    float* out;                     /* (B, 3C+3, V) dense: written by the forward */
    void* workspace;                /* mm_shape_features_query_workspace bytes: scratch of the backward, unused by the forward */
    size_t workspace_bytes;
} MMShapeFeatDesc;
typedef struct MMShapeFeatGrads {
    const float* grad_out;          /* (B, 3C+3, V) dense */
    void* grad_x;                   /* (B,C,H,W) dense in x_dtype, every element overwritten, or NULL */
    float* grad_p;                  /* (1) overwritten, or NULL; not both NULL */
} MMShapeFeatGrads;
typedef struct MMCameraFeatDesc {
    int32_t B, C, H, W, V;          /* limits as MMShapeFeatDesc */
    int32_t x_dtype;
    const void* x;
    int64_t x_strides[4];
    const float* template_xyz;      /* (V,3) dense; columns 0, 1 sample */
    const float* p_map;             /* (1) MMPool.p of the pool over x */
    const float* p_local;           /* (1) MMPool.p of the pool over the sampled (V,1) map */
    float* out;                     /* (B, 2C, 2, 2) dense */
    void* workspace;                /* mm_camera_features_query_workspace bytes: scratch of the backward */
    size_t workspace_bytes;
} MMCameraFeatDesc;
typedef struct MMCameraFeatGrads {
    const float* grad_out;          /* (B, 2C, 2, 2) dense */
    void* grad_x;                   /* (B,C,H,W) dense in x_dtype, or NULL */
    float* grad_p_map;              /* (1), or NULL */
    float* grad_p_local;            /* (1), or NULL; not all three NULL */
} MMCameraFeatGrads;
/* bytes of workspace the backward of this shape needs; 0 for a bad shape */
size_t mm_shape_features_query_workspace(const MMShapeFeatDesc* desc);
int mm_shape_features_forward(const MMShapeFeatDesc* desc, mm_stream_t stream);
int mm_shape_features_backward(const MMShapeFeatDesc* desc, const MMShapeFeatGrads* grads, mm_stream_t stream);
size_t mm_camera_features_query_workspace(const MMCameraFeatDesc* desc);
int mm_camera_features_forward(const MMCameraFeatDesc* desc, mm_stream_t stream);
int mm_camera_features_backward(const MMCameraFeatDesc* desc, const MMCameraFeatGrads* grads, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Attribute interpolation: the block the reference's generator step runs between its first and second render
 * (trainer.py:293-342).  For every output row j of each of the five attribute tensors:
 *   out[j] = fl(fl(a[j] * src[ia[j]]) + fl(fl(1 - a[j]) * src[ib[j]]))     (every operation rounded in fp32: torch's eager result)
 * with a = alpha_shape for vertices and delta_vertices, alpha_texture for textures and bg, alpha_light for lights.  A row whose ia
 * or ib lies outside [0, B) is written as NaN and nothing is read for it.  The backward gives source row i
 *   sum over j with ia[j] == i, ascending, of fl(a[j] * g[j]), then over j with ib[j] == i, ascending, of fl(fl(1 - a[j]) * g[j]),
 * accumulated left to right from +0.0 (rows nobody selected: 0).  No float atomics; bitwise reproducible.  The forward is one
 * launch and needs no workspace; the backward builds the inverse index lists in the workspace (one small launch) and gathers.
 * B <= 65535 (MM_ERR_UNSUPPORTED otherwise).  All tensors fp32, dense, rows contiguous.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct MMInterpDesc {
    int32_t B, V, Ht, Wt, H, W;     /* H, W are read only when bg (forward) or bg's gradient pair (backward) is given */
    const float* vertices;          /* (B,V,3) */
    const float* delta_vertices;    /* (B,V,3) */
    const float* textures;          /* (B,3,Ht,Wt) */
    const float* bg;                /* (B,3,H,W), or NULL */
    const float* lights;            /* (B,9) */
    float* out_vertices;            /* outputs of the forward, shaped like the sources */
    float* out_delta_vertices;
    float* out_textures;
    float* out_bg;                  /* ignored when bg is NULL */
    float* out_lights;
    const int32_t* idx_a;           /* (B) device: the row each output row takes with weight a */
    const int32_t* idx_b;           /* (B) device: ... with weight 1 - a */
    const float* alpha_shape;       /* (B) */
    const float* alpha_texture;     /* (B) */
    const float* alpha_light;       /* (B) */
    void* workspace;                /* mm_interp_query_workspace bytes: scratch of the backward, unused by the forward */
    size_t workspace_bytes;
} MMInterpDesc;
typedef struct MMInterpGrads {
    /* per tensor an upstream gradient (shaped like the output) and the source gradient it produces (overwritten), both given or both
     * NULL; a NULL pair is skipped (no launch at all when all five are).  The backward reads none of the sources. */
    const float* grad_out_vertices;
    const float* grad_out_delta_vertices;
    const float* grad_out_textures;
    const float* grad_out_bg;
    const float* grad_out_lights;
    float* grad_vertices;
    float* grad_delta_vertices;
    float* grad_textures;
    float* grad_bg;
    float* grad_lights;
} MMInterpGrads;
/* bytes of workspace the backward needs for this B; 0 for a bad shape */
size_t mm_interp_query_workspace(const MMInterpDesc* desc);
/* Collapse resampling, one launch: bad[b] = ((|x| + |y|) + |z|) / 3 > threshold over the last vertex of delta_vertices (B,V,3),
 * in fp32; a NaN mean is not bad.  good = the samples that are not bad, ascending.  Every slot s of idx_a holding a bad sample is
 * set to good[min(floor(fl(uniforms[s] * n_good)), n_good - 1)], and every such slot of idx_b to the same with uniforms[B + s]
 * (uniforms: (2,B) in [0, 1)).  Indices outside [0, B) are left as they are.  *n_bad (device int) = the number of bad samples; when
 * every sample is bad the indices are left unchanged and *n_bad = B. */
int mm_collapse_resample(int32_t B, int32_t V, const float* delta_vertices, int32_t* idx_a, int32_t* idx_b, const float* uniforms,
                         float threshold, int32_t* n_bad, mm_stream_t stream);
int mm_attribute_mix_forward(const MMInterpDesc* desc, mm_stream_t stream);
int mm_attribute_mix_backward(const MMInterpDesc* desc, const MMInterpGrads* grads, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Critic inputs: the image batches the reference's GAN step assembles for its discriminator (trainer.py:370-411, 429-431).
 * With the channel map M of the unmask mode (C output channels; m = X[:, 3]):
 *   unmask 0 (C = 3): M(X)_c = fl(fl(X_c * m) + fl(1 - m))     the image over white with its own alpha
 *   unmask 1 (C = 3): M(X)_c = X_c
 *   unmask 2 (C = 4): M(X)   = X
 * the forward writes, in one launch,
 *   out_batch   (3B,C,H,W) = cat(M(Xa), M(Xer90), M(Xir)) -- the D step's batch; its rows [B, 3B) are the G step's batch
 *   out_gp_er90 (B,C,H,W)  = fl(fl(a1 * M(Xa)) + fl(fl(1 - a1) * M(Xer90)))     (only when the alphas are given)
 *   out_gp_ir   (B,C,H,W)  = fl(fl(a2 * M(Xa)) + fl(fl(1 - a2) * M(Xir)))
 * every operation rounded in fp32: torch's eager results.  The backward takes the (2B,C,H,W) gradient of rows [B, 3B) and writes,
 * in one launch, the gradients of Xer90 and Xir, each (B,4,H,W) in the layout its flag names:
 *   unmask 0: d X_c = fl(g_c * m), d m = ((g_0 * (X_0 - 1)) + g_1 * (X_1 - 1)) + g_2 * (X_2 - 1)
 *   unmask 1: d X_c = g_c, d m = 0          unmask 2: d X = g
 * No atomics, no workspace; bitwise reproducible.  Inputs and gradients are fp32 (B,4,H,W), each either NCHW-contiguous (flag 0)
 * or NHWC-dense, strides (4HW, 1, 4W, 4) (flag 1: what mm_render_forward writes); the outputs and g_batch are NCHW-contiguous.
 * H * W a multiple of 4 and 16-byte aligned pointers move 16 bytes per access, anything else 4.  Xa takes no gradient.
 * 2 * B * ceil(H * W / 256) must fit an int32 (MM_ERR_UNSUPPORTED otherwise).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct MMCriticDesc {
    int32_t B, H, W, unmask;        /* unmask: 0, 1 or 2 (MM_ERR_BAD_SHAPE otherwise) */
    const float* Xa;                /* (B,4,H,W) the real images; the backward does not read them (may be NULL there) */
    const float* Xer90;             /* (B,4,H,W) the first fake; the backward reads the fakes for unmask 0 only */
    const float* Xir;               /* (B,4,H,W) the second fake; may be the same memory as Xer90 */
    int32_t Xa_nhwc, Xer90_nhwc, Xir_nhwc;   /* layout flag of each input */
    const float* alpha_er90;        /* (B) a1, or NULL: then alpha_ir is NULL too and no interpolate is written */
    const float* alpha_ir;          /* (B) a2 */
    float* out_batch;               /* (3B,C,H,W); forward only */
    float* out_gp_er90;             /* (B,C,H,W); forward with alphas only */
    float* out_gp_ir;
} MMCriticDesc;
typedef struct MMCriticGrads {
    const float* g_batch;           /* (2B,C,H,W) upstream gradient of out_batch's rows [B, 3B) */
    float* grad_er90;               /* (B,4,H,W), overwritten; NULL: not wanted (both NULL: no launch) */
    float* grad_ir;
    int32_t grad_er90_nhwc, grad_ir_nhwc;    /* layout flag of each gradient */
} MMCriticGrads;
int mm_critic_inputs_forward(const MMCriticDesc* desc, mm_stream_t stream);
int mm_critic_inputs_backward(const MMCriticDesc* desc, const MMCriticGrads* grads, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Export: float renders to 8-bit pixels on the device (what the reference's evaluation code does on the host: to_pil_image,
 * make_grid + permute + (image * 255).astype(uint8), save_image; trainer.py:546-769).  The quantiser, every step rounded in fp32:
 *   rounding 0 (trunc):   q = fl(x * 255)               -- pic.mul(255).byte(), (image * 255.0).astype(np.uint8)
 *   rounding 1 (nearest): q = fl(fl(x * 255) + 0.5)     -- save_image
 * then NaN -> 0, clamp to [0, 255], convert toward zero.  For x outside [0, 1] the reference's cast is undefined; this one SATURATES.
 * white (C = 4 only) first composes the pixel over white with its own alpha: x_c <- fl(fl(x_c * m) + fl(1 - m)), m = x_3.
 * The input is B * N images of (C,H,W) fp32, C 3 or 4, image b * N + n after image b * N + n - 1: NCHW-contiguous (nhwc 0) or, for
 * C = 4, NHWC-dense (nhwc 1: what mm_render_forward and mm_render_views_forward write).
 * mm_export_images writes any subset of out_rgb (B*N,H,W,3), out_mask (B*N,H,W) -- channel 3 --, out_rgba (B*N,H,W,4) as bytes in one
 * launch from one read of each pixel; with as_float the same quantised values as fp32 fl(float(q) / 255) in planes: (B*N,3,H,W),
 * (B*N,H,W), (B*N,4,H,W).  mm_export_grid writes out_grid (N,Hg,Wg,3) bytes, frame n = torchvision's
 * make_grid(x[:, n, :3], nrow, padding, pad_value) in HWC, all frames in one launch: for B = 1 the image itself (Hg = H, Wg = W),
 * otherwise xmaps = min(nrow, B), ymaps = ceil(B / xmaps), Hg = (H + padding) * ymaps + padding, Wg = (W + padding) * xmaps + padding,
 * image k = y * xmaps + x at rows [y * (H + padding) + padding, ... + H) and columns [x * (W + padding) + padding, ... + W), every
 * other byte (the empty cells of a short last row too) the quantised pad_value.
 * No atomics, no workspace, no host synchronisation; bitwise reproducible.  16-byte aligned pointers move 16 bytes per access.  The
 * 16-byte chunks of an output are counted in an int32 (MM_ERR_UNSUPPORTED otherwise).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct MMExportDesc {
    int32_t B, N, C, H, W;          /* B * N images; grid mode: B cells per frame, N frames */
    int32_t nhwc;                   /* layout flag of x; 1 needs C = 4 (MM_ERR_BAD_SHAPE otherwise) */
    int32_t rounding;               /* 0 trunc, 1 nearest (MM_ERR_BAD_SHAPE otherwise) */
    int32_t white;                  /* compose over white first; needs C = 4 */
    int32_t as_float;               /* mm_export_images only: fp32 planes instead of bytes */
    int32_t nrow, padding;          /* mm_export_grid only: nrow >= 1, padding >= 0 */
    float pad_value;                /* mm_export_grid only */
    const float* x;
    void* out_rgb;                  /* mm_export_images: each NULL or an output; at least one */
    void* out_mask;                 /* needs C = 4 */
    void* out_rgba;                 /* needs C = 4 */
    uint8_t* out_grid;              /* mm_export_grid */
} MMExportDesc;
int mm_export_images(const MMExportDesc* desc, mm_stream_t stream);
int mm_export_grid(const MMExportDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Batch assembly: training batches (B,4,H,W) fp32 from device-resident 8-bit images, what the reference's DataLoader workers do per
 * sample in Pillow (datasets/bird.py:69-136, datasets/market.py:77-145), in one launch.  The decoded images lie packed in `images`
 * (rgb bytes, image i at byte 3 * offsets[i]) and `segs` (one byte per pixel, image i at byte offsets[i]) without padding; sizes holds
 * rows (H_i, W_i).  Each sample is one canonical record of 16 int32:
 *    0 img        source image
 *    1 flip_src   read the source mirrored in x; the coordinates below are in the mirrored image
 *    2 x0  3 y0  4 Wc  5 Hc     the canvas window, which may hang over any edge
 *    6 cx0 7 cy0 8 cx1 9 cy1    the clip rectangle [cx0,cx1) x [cy0,cy1): a canvas pixel outside it or outside the image is 0 (rgb and mask)
 *   10 Wr 11 Hr   the canvas is resized to (Wr,Hr): rgb by Pillow's antialiased bicubic (22-bit fixed point, the horizontal pass to
 *                 clamped bytes, then the vertical pass), the mask by Pillow's nearest, then 255 if m > 160 else 0
 *   12 dx 13 dy   output pixel (x,y) reads resized (x + dx, y + dy), 0 outside
 *   14 flip_out   ... of the output mirrored in x: resized (W - 1 - x + dx, y + dy)
 *   15 reserved
 * then v = fl(q / 255); rgb = m ? v : 1.0 unless bg; channel 3 = m as 0.0 / 1.0.  out is dense NCHW.
 * records_host is the host's copy of the device table `records` (the caller uploads it, e.g. one non-blocking copy from pinned memory):
 * it is validated and sizes the kernel's LDS before anything is launched.  MM_ERR_BAD_SHAPE: B, H, W, n_images < 1, img outside
 * [0, n_images), Wc, Hc, Wr or Hr < 1, a flag that is not 0 / 1, a coordinate beyond +-2^24.  MM_ERR_UNSUPPORTED: Wc > MM_BATCH_MAX_RATIO * Wr
 * or Hc > MM_BATCH_MAX_RATIO * Hr (any upscale is allowed), B > 65535, or tap tables and row buffer beyond the 160 KiB of LDS:
 *   4 * (Wr * ksx + MM_BATCH_ROWS * ksy + 3 * Wr + 3 * MM_BATCH_ROWS) + 3 * Wr * rows bytes (rounded up to 4), with per axis
 *   ks = 2 * ceil(2 * max(in / out, 1)) + 1 and rows = floor((MM_BATCH_ROWS - 1) * Hc / Hr) + ksy + 1, each the largest of the batch:
 *   1024 -> 128 (8:1) takes 53 KiB; at 16:1 outputs at least 190 wide fit.
 * No workspace, no atomics, no host synchronisation; bitwise reproducible.  Not differentiable.
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_BATCH_MAX_RATIO 16
#define MM_BATCH_ROWS 8             /* output rows per workgroup */
typedef struct MMBatchDesc {
    int32_t B, H, W;                /* the output batch (B,4,H,W) */
    int32_t n_images;               /* images in the pool */
    int32_t bg;                     /* keep the background: rgb = v everywhere */
    int32_t reserved;
    const uint8_t* images;
    const uint8_t* segs;
    const int64_t* offsets;         /* (n_images) pixel offsets */
    const int32_t* sizes;           /* (n_images,2) rows (H_i, W_i) */
    const int32_t* records_host;    /* (B,16), host memory */
    const int32_t* records;         /* (B,16), device memory, the same values */
    float* out;
} MMBatchDesc;
int mm_assemble_batch(const MMBatchDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Composite: renders composed over blurred backgrounds as 8-bit frames, what the reference's dataset-generation scripts do on the host per
 * image after every render (generate_market++.py:308-349, generate_market_new_class9.py:323-347, tool/generate_market.py:293-313), in one
 * launch: B frames (B,H,W,3) bytes -- or, with as_float, (B,3,H,W) fp32 planes fl(float(q) / 255) -- from `renders`, n_fg images (4,H,W)
 * fp32, NCHW-contiguous (fg_nhwc 0) or NHWC-dense (fg_nhwc 1: what mm_render_forward and mm_render_views_forward write), and
 * `backgrounds`, n_bg images (bg_C,H,W) fp32 NCHW-contiguous, bg_C 3 or 4, of which channels 0-2 are read.  Per frame o, all in fp32,
 * every operation rounded as written, every sum taken in ascending tap index starting from 0:
 *   mask      m = channel 3 of render fg_index[o].  fill_holes: s = the sum of the 3x3 neighbourhood's pixels inside the image, row by row,
 *             s = fl(s / 9), then 1 if s > 0.7, 0 if s <= 0.7 (NaN stays).  Blur: sum_j fl(k[j] * m[R(x + j - r)]) along x, then the same
 *             along y, k = the frame's mask_k taps, r = (mask_k - 1) / 2, R reflecting at the image's edge.  mask_pad p: the blurred mask
 *             replicate-padded by p and resized (H + 2p, W + 2p) -> (H,W): sum_t fl(w[x][t] * b[C(start[x] + t - p)]) along x, then along y.
 *   bg        plane c of background bg_index[o] behind the reflection pad bg_pad = (left, right, top, bottom): a virtual image
 *             (H + top + bottom, W + left + right) that is index arithmetic only; blurred with the frame's bg_k taps, reflecting at the
 *             VIRTUAL image's edge (an index may be reflected twice); resized to (H,W) like the mask.
 *   blend     out_c = fl(fl(fg_c * m') + fl(bg'_c * fl(1 - m'))), fg_c = channel c of the render, then the Export quantiser above,
 *             unchanged: rounding 0 trunc / 1 nearest, NaN -> 0, saturating.
 * A stage a caller does not want is the identity in this form: one blur tap of 1.0; a resize row {start i, 1 tap, 1.0}.
 * params is ONE table of 32-bit words (floats by their bits) that the caller uploads; params_host is the host's copy of it, which is
 * validated and sizes the kernel's LDS before anything is launched:
 *   fg_index (B) | bg_index (B) | mask taps (B,mask_k) | bg taps (B,bg_k) | resize rows: mask y (H), mask x (W), bg y (H), bg x (W)
 * a resize row being MM_COMPOSITE_ROW_WORDS words {start, n, w[0..8)}: output index i reads inputs [start, start + n) of the padded axis.
 * MM_ERR_BAD_SHAPE: B, H, W, n_fg, n_bg < 1; bg_C not 3 or 4; a kernel that is even, < 1 or > MM_COMPOSITE_MAX_KERNEL; a negative pad; a
 * reflection pad >= the dimension it reflects in, a blur radius >= the (virtual) dimension it reflects in; an index outside [0, n_fg) /
 * [0, n_bg); a resize row with n outside [1, MM_COMPOSITE_MAX_TAPS] or taps outside the padded axis; rounding not 0 / 1.
 * MM_ERR_UNSUPPORTED: more than the 160 KiB of LDS -- 8 * (rows * width of the largest plane of any band: the blurred rows its vertical
 * taps read + kernel - 1, times the virtual width) + 4 * MM_COMPOSITE_ROWS * W + 24 * W + 32 bytes, rounded up; kernel 31 behind a pad of 16 at 128 x 128
 * takes 60 KiB, kernel 5 at 128 x 64 behind (8,8,16,16) 14 KiB --, or more than 2^31 - 1 workgroups.
 * No workspace, no atomics, no host synchronisation; bitwise reproducible.  Not differentiable.
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_COMPOSITE_ROWS 8         /* output rows per workgroup */
#define MM_COMPOSITE_MAX_KERNEL 31
#define MM_COMPOSITE_MAX_TAPS 8     /* resize taps per output index */
#define MM_COMPOSITE_ROW_WORDS 10
typedef struct MMCompositeDesc {
    int32_t B, H, W;                /* the frames */
    int32_t n_fg, n_bg, bg_C;       /* images in renders / backgrounds; channels of a background */
    int32_t fg_nhwc;                /* layout flag of renders */
    int32_t fill_holes;
    int32_t mask_k, bg_k;           /* blur taps per frame: odd, 1 = none (the tap is 1.0) */
    int32_t mask_pad;               /* replicate pad of the blurred mask before its resize */
    int32_t bg_pad[4];              /* reflection pad of the background: left, right, top, bottom */
    int32_t rounding;               /* 0 trunc, 1 nearest */
    int32_t as_float;               /* fp32 planes (B,3,H,W) instead of bytes (B,H,W,3) */
    int32_t reserved;
    const float* renders;
    const float* backgrounds;
    const int32_t* params_host;     /* host memory */
    const int32_t* params;          /* device memory, the same words */
    void* out;
} MMCompositeDesc;
int mm_composite_frames(const MMCompositeDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Pyramid: renders blended into backgrounds through a three-level Laplacian pyramid as 8-bit frames, what the reference's
 * tool/generate_market_test.py:326-369 does on the host per image after every render, in one launch: B frames (B,H,W,3) bytes -- or,
 * with as_float, (B,3,H,W) fp32 planes fl(float(q) / 255) -- from `renders` and `backgrounds` as MMCompositeDesc takes them.  Per frame
 * o there are three plane KINDS, 0 the mask, 1 the background, 2 the render, and every plane is blurred MM_PYRAMID_LEVELS = 3 times in a
 * cascade, level l with the frame's own taps[o][kind][l - 1].  All in fp32, every operation rounded as written, every sum taken in
 * ascending tap index starting from 0, no contraction:
 *   level 0   m0 = channel 3 of render fg_index[o]; obj0_c = its channel c, untouched; bg0_c = plane c of background bg_index[o] behind
 *             the reflection pad bg_pad = (left, right, top, bottom) -- a virtual image (H + top + bottom, W + left + right) that is index
 *             arithmetic only -- resized to (H,W): sum_t fl(w[x][t] * v[C(start[x] + t)]) along x, then the same along y, C clamping to
 *             the virtual image.  There is NO blur before the resize (the reference's order at this call site).
 *   level l   v_l = vblur(hblur(v_{l-1})): sum_j fl(k[j] * v[R(x + j - r)]) along x, then the same along y, r = (k - 1) / 2, R reflecting
 *             at the (H,W) image's own edge, at every level.
 *   blend     t = fl(bg3 * fl(1 - m3)); t = fl(t + fl(obj3 * m3)); t = fl(t + fl(fl(bg1 - bg2) * fl(1 - m2)));
 *             t = fl(t + fl(fl(obj1 - obj2) * m2)); t = fl(t + fl(fl(bg0 - bg1) * fl(1 - m1))); t = fl(t + fl(fl(obj0 - obj1) * m1)),
 *             then the Export quantiser above, unchanged: rounding 0 trunc / 1 nearest, NaN -> 0, saturating (the sums leave [0, 1]).
 * A one-tap kernel {1.0} makes a level the identity; resize rows {start i, 1 tap, 1.0} make level 0 of the background the image itself.
 * params is ONE table of 32-bit words (floats by their bits) that the caller uploads; params_host is the host's copy of it, which is
 * validated and sizes the kernel's LDS before anything is launched:
 *   fg_index (B) | bg_index (B) | taps (B,3,3,k): [frame][kind][level] | resize rows: bg y (H), bg x (W)
 * a resize row being MM_PYRAMID_ROW_WORDS words {start, n, w[0..8)}: output index i reads inputs [start, start + n) of the padded axis.
 * MM_ERR_BAD_SHAPE: B, H, W, n_fg, n_bg < 1; bg_C not 3 or 4; k even, < 1 or > MM_PYRAMID_MAX_KERNEL; a pad that is negative or >= the
 * dimension it reflects in; a radius >= min(H, W); an index outside [0, n_fg) / [0, n_bg); a resize row with n outside
 * [1, MM_PYRAMID_MAX_TAPS] or taps outside the padded axis; rounding not 0 / 1.
 * MM_ERR_UNSUPPORTED: more than the 160 KiB of LDS -- 8 * rows * W (rows: the most any band of MM_PYRAMID_ROWS stages, 8 + 3 (k - 1) of
 * level 0 or the padded rows their vertical taps read) + 320 * W + 24 * W + 32 bytes, rounded up; kernel 7 behind a pad of 16 takes 39 KiB
 * at 128 x 64, 77 KiB at 128 x 128 and 148 KiB at 256 x 256 --, or more than 2^31 - 1 workgroups.
 * No workspace, no atomics, no host synchronisation; bitwise reproducible.  Not differentiable.
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_PYRAMID_ROWS 8           /* output rows per workgroup */
#define MM_PYRAMID_LEVELS 3
#define MM_PYRAMID_MAX_KERNEL 15    /* LDS does not force less: kernel 15 at 128 x 128 behind a pad of 16 takes 107 KiB */
#define MM_PYRAMID_MAX_TAPS 8       /* resize taps per output index */
#define MM_PYRAMID_ROW_WORDS 10
typedef struct MMPyramidDesc {
    int32_t B, H, W;                /* the frames */
    int32_t n_fg, n_bg, bg_C;       /* images in renders / backgrounds; channels of a background */
    int32_t fg_nhwc;                /* layout flag of renders */
    int32_t k;                      /* blur taps per frame, kind and level: odd, 1 = none (the tap is 1.0) */
    int32_t bg_pad[4];              /* reflection pad of the background: left, right, top, bottom */
    int32_t rounding;               /* 0 trunc, 1 nearest */
    int32_t as_float;               /* fp32 planes (B,3,H,W) instead of bytes (B,H,W,3) */
    const float* renders;
    const float* backgrounds;
    const int32_t* params_host;     /* host memory */
    const int32_t* params;          /* device memory, the same words */
    void* out;
} MMPyramidDesc;
int mm_pyramid_frames(const MMPyramidDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Poisson: renders blended into backgrounds by Poisson (seamless-cloning) editing as 8-bit frames -- the system the reference's
 * poisson_image_editing.py:33-108 builds with offset (0,0) and solves with one sparse direct solve per frame and channel on the host --
 * in one launch: B frames (B,H,W,3) bytes, or, with as_float, (B,3,H,W) fp32 planes fl(float(q) / 255), from `renders` and `backgrounds`
 * as MMCompositeDesc takes them.  Per frame o and colour channel c, all in fp32, every operation rounded as written, no contraction:
 *   s         channel c of render fg_index[o], untouched
 *   t         plane c of background bg_index[o] behind the reflection pad bg_pad, resized to (H,W): level 0 of MMPyramidDesc's
 *             background, bit for bit (x, then y, taps ascending from 0, no blur)
 *   in        mask[fg_index[o]][y][x] != 0 if mask is given (bytes (n_fg,H,W)); otherwise the Export quantiser's trunc byte of the
 *             render's channel 3 != 0
 *   pinned    x = t.  border 0 ("reference"): the cells outside the mask that are not on the image's outer row or column;
 *             border 1 ("pinned"): every cell outside the mask.
 *   free      every other cell: 4 x_p - sum x_q = b_p over the 4-neighbours q inside the image; inside the mask
 *             b = fl(fl(4 s) - fl(fl(sl + sr) + fl(su + sd))) with a neighbour outside the image as 0; outside it (the outer-border cells
 *             of border 0) b = t.
 *   solve     x = t everywhere; then `sweeps` red-black SOR sweeps, the free cells with (y + x) even first, then those with (y + x) odd:
 *             x <- fl(x + fl(omega * fl(fl(fl(b + fl(fl(l + r) + fl(u + d))) * 0.25) - x))), a neighbour outside the image read as 0.
 *             Cells of one colour do not read each other.  The sweep count is fixed: no convergence test, nothing comes back.
 *   quantise  the Export quantiser above, unchanged: rounding 0 trunc / 1 nearest, NaN -> 0, saturating (the solution leaves [0, 1]).
 * params is ONE table of 32-bit words (floats by their bits) that the caller uploads; params_host is the host's copy of it, which is
 * validated and sizes the kernel's LDS before anything is launched:
 *   fg_index (B) | bg_index (B) | resize rows: bg y (H), bg x (W)
 * a resize row being MM_PYRAMID_ROW_WORDS words {start, n, w[0..8)} as in MMPyramidDesc.
 * MM_ERR_BAD_SHAPE: B, H, W, n_fg, n_bg < 1; bg_C not 3 or 4; a pad that is negative or >= the dimension it reflects in; an index
 * outside [0, n_fg) / [0, n_bg); a resize row with n outside [1, MM_PYRAMID_MAX_TAPS] or taps outside the padded axis; rounding or border
 * not 0 / 1; sweeps < 0 or > MM_POISSON_MAX_SWEEPS; omega not inside (0, 2).
 * MM_ERR_UNSUPPORTED: more than the 160 KiB of LDS -- one workgroup holds a whole plane for the whole solve: 8 * (H + 2) * ((W + 3) / 2)
 * + 4 * rows * W bytes (rows: the most source rows the vertical resize of 8 output rows reads), each term rounded up to 16;
 * 36 896 bytes at 128 x 64 and 72 736 at 128 x 128 behind a pad of 16; 256 x 256 does not fit --, or more than 2^31 - 1 workgroups.
 * No workspace, no atomics, no host synchronisation; bitwise reproducible.  Not differentiable.
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_POISSON_MAX_SWEEPS (1 << 16)
typedef struct MMPoissonDesc {
    int32_t B, H, W;                /* the frames */
    int32_t n_fg, n_bg, bg_C;       /* images in renders / backgrounds; channels of a background */
    int32_t fg_nhwc;                /* layout flag of renders */
    int32_t border;                 /* 0 reference: outer-border cells outside the mask are free; 1 pinned: they keep t */
    int32_t bg_pad[4];              /* reflection pad of the background: left, right, top, bottom */
    int32_t rounding;               /* 0 trunc, 1 nearest */
    int32_t as_float;               /* fp32 planes (B,3,H,W) instead of bytes (B,H,W,3) */
    int32_t sweeps;                 /* red-black sweeps, >= 0 */
    float omega;                    /* the relaxation factor, inside (0, 2) */
    const float* renders;
    const float* backgrounds;
    const uint8_t* mask;            /* NULL, or (n_fg,H,W) bytes: non-zero is inside */
    const int32_t* params_host;     /* host memory */
    const int32_t* params;          /* device memory, the same words */
    void* out;
} MMPoissonDesc;
int mm_poisson_frames(const MMPoissonDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * JPEG: n device frames (n,H,W,3) of bytes -- what mm_export_images, mm_composite_frames and mm_pyramid_frames write, at any byte
 * alignment -- as n complete baseline JPEG files, byte for byte what libjpeg(-turbo) writes for 4:2:0 with the standard Huffman tables,
 * the islow DCT and quantisation tables q (Pillow's Image.save(f, 'JPEG', quality=...)).  The caller writes the file's head, SOI up to and
 * including SOS, and gives the tables; everything after SOS is made on the device.  Integer arithmetic only (>> arithmetic):
 *   colour    Y = (19595 R + 38470 G + 7471 B + 32768) >> 16; Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16;
 *             Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *   edges     an MCU is 16 x 16 pixels, blocks Y00 Y01 Y10 Y11 Cb Cr.  Columns beyond W replicate the input's last column, rows beyond H
 *             its last row up to an even height; chroma rows beyond ceil(H / 2) replicate the DOWNSAMPLED last row.  A luma block wholly
 *             beyond ceil(W / 8) or ceil(H / 8) is a dummy: no AC, the DC of the block before it in MCU order.
 *   chroma    (a + b + c + d + bias) >> 2 over 2 x 2, bias 1 on even output columns and 2 on odd ones
 *   DCT       jfdctint (islow) on the samples minus 128, CONST_BITS 13, PASS1_BITS 2, rows then columns; the output is scaled by 8
 *   quantise  sign(v) * ((|v| + (d >> 1)) / d) with the divisor d = 8 * q: half away from zero
 *   entropy   MCUs in raster order, a DC predictor per component, ZRL for sixteen zeros, EOB unless coefficient 63 is non-zero, the last
 *             byte padded with 1-bits, 0x00 after every 0xFF, then EOI.
 * params is ONE table of 32-bit words that the caller uploads; params_host is the host's copy of it, validated before anything is
 * launched:   divisors (2,64): luma, chroma, NATURAL order, each 8 * q with q in 1..255
 *           | codes (4,256): DC luma, AC luma, DC chroma, AC chroma, per symbol size << 16 | code (0: no such symbol)
 *           | the file's head, header_bytes bytes in file order, padded to a word.
 * The workspace is the caller's, mm_jpeg_query_workspace bytes, 16-byte aligned; the library allocates nothing.  After the call it holds
 * the results: at byte 0 offsets[n + 1] as int64, and from byte mm_jpeg_files_offset on the files back to back, file i being bytes
 * [offsets[i], offsets[i + 1]) of that region: a caller copies the offsets, then exactly offsets[n] bytes.  The rest is scratch:
 * int16 coefficients (128 bytes per block, six blocks per MCU), a bit count per block, the unstuffed streams at MM_JPEG_BLOCK_BYTES per
 * block (a block codes to 20 + 63 * 26 bits at most) in whole chunks of MM_JPEG_CHUNK_BYTES, and a count per chunk; a file has room for
 * header_bytes + twice its stream + 2.  A stream is never held in LDS.
 * MM_ERR_BAD_SHAPE: n, H, W < 1; header_bytes outside [2, MM_JPEG_MAX_HEADER]; a divisor that is not 8 * (1..255); a code wider than its
 * size or than 16 bits, or whose size plus category bits (symbol & 15) exceeds 26.  MM_ERR_UNSUPPORTED: H, W or n > 65535; more than MM_JPEG_MAX_BLOCKS blocks in a frame or 2^30 in a call (the
 * queries return 0).  MM_ERR_WORKSPACE: too small or misaligned.
 * Nine stream operations (one memset, eight launches), no host synchronisation; bitwise reproducible.
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_JPEG_BLOCK_BYTES 208
#define MM_JPEG_CHUNK_BYTES 1024
#define MM_JPEG_MAX_BLOCKS (1 << 20)
#define MM_JPEG_MAX_HEADER 4096
typedef struct MMJpegDesc {
    int32_t n, H, W;                /* the frames */
    int32_t header_bytes;           /* bytes of the file's head in params */
    const uint8_t* frames;          /* (n,H,W,3), dense, any alignment */
    const int32_t* params_host;     /* host memory */
    const int32_t* params;          /* device memory, the same words */
    void* workspace;
    size_t workspace_bytes;
} MMJpegDesc;
size_t mm_jpeg_query_workspace(const MMJpegDesc* desc);     /* reads n, H, W, header_bytes */
size_t mm_jpeg_files_offset(const MMJpegDesc* desc);        /* where the files start in the workspace */
int mm_jpeg_encode(const MMJpegDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * JPEG, every layout: mm_jpeg_encode with the MCU as a parameter -- the files Pillow's save(f, 'JPEG', quality=q, subsampling=s) writes
 * of an (H,W,3) frame for s = 4:2:0, 4:2:2 and 4:4:4, and the greyscale file it writes of an (H,W) frame.  MMJpegDesc and mm_jpeg_* are
 * this with mode RGB and sampling 4:2:0 (they forward here).  Colour conversion, DCT, quantiser, entropy coder, padding, stuffing and EOI
 * are mm_jpeg_encode's; the layouts differ in the MCU alone:
 *   4:2:0      16 x 16 pixels, blocks Y00 Y01 Y10 Y11 Cb Cr: above.
 *   4:2:2      16 wide, 8 high, blocks Y0 Y1 Cb Cr.  Columns beyond W replicate the input's last column up to the MCU, rows beyond H its last
 *              row up to the block.  Chroma is (c[2x] + c[2x+1] + bias) >> 1, bias 0 on even output columns and 1 on odd ones.  Y1 is a
 *              dummy (no AC, Y0's DC) where 2 mx + 1 >= ceil(W / 8).  No vertical dummy and no downsampled-row rule.
 *   4:4:4      8 x 8 pixels, blocks Y Cb Cr, edges replicated on all three planes; no downsampling, no dummies.
 *   greyscale  mode L: frames are (n,H,W).  A non-interleaved scan: an MCU is one 8 x 8 block, ceil(H / 8) x ceil(W / 8) of them in raster
 *              order, edges replicated, no dummies; the luma divisors, the luma tables, one DC predictor.
 * params is MMJpegDesc's table in every layout (both divisor tables and all four code tables, whichever the layout reads); the file's
 * head differs: a greyscale head has one DQT, a one-component SOF0 and SOS and the two luma DHT segments; a colour head has Y's sampling
 * byte 0x22, 0x21 or 0x11.  The workspace is laid out as mm_jpeg_encode's, counted in the layout's own blocks (6, 4, 3 or 1 per MCU).
 * Return codes as mm_jpeg_encode's; MM_ERR_BAD_SHAPE also for an unknown mode or sampling and for a sampling other than 0 with mode L;
 * the block limits of MM_ERR_UNSUPPORTED count the layout's own blocks.  Every refusal comes before any GPU work.
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_JPEG_SAMPLING_420 0
#define MM_JPEG_SAMPLING_422 1
#define MM_JPEG_SAMPLING_444 2
typedef struct MMJpegModesDesc {
    int32_t n, H, W;                /* the frames */
    int32_t header_bytes;           /* bytes of the file's head in params */
    int32_t mode;                   /* MM_JPEG_MODE_RGB or MM_JPEG_MODE_L (below) */
    int32_t sampling;               /* MM_JPEG_SAMPLING_*; 0 with mode L */
    const uint8_t* frames;          /* (n,H,W,3), or (n,H,W) in mode L; dense, any alignment */
    const int32_t* params_host;     /* host memory */
    const int32_t* params;          /* device memory, the same words */
    void* workspace;
    size_t workspace_bytes;
} MMJpegModesDesc;
size_t mm_jpeg_modes_query_workspace(const MMJpegModesDesc* desc);      /* reads n, H, W, header_bytes, mode, sampling */
size_t mm_jpeg_modes_files_offset(const MMJpegModesDesc* desc);         /* where the files start in the workspace */
size_t mm_jpeg_modes_coef_offset(const MMJpegModesDesc* desc);          /* where the coefficients lie in it, for mm_jpeg_roundtrip */
int mm_jpeg_modes_encode(const MMJpegModesDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * JPEG round trip: n device frames as a decoder reads them back from the files above -- to the byte what Pillow's
 * Image.open(file).convert('RGB') gives for mm_jpeg_encode's file of an (H,W,3) frame (mode RGB, 4:2:0), and what
 * Image.open(file).convert('L') gives for the greyscale file libjpeg writes of an (H,W) frame (mode L; that file is never formed).  No
 * entropy decoder: a file's content is its quantised coefficients.  Integer arithmetic only (>> arithmetic), libjpeg's decoder:
 *   dequantise  c[k] * table[k], table = divisor / 8 (luma for Y and greyscale, chroma for Cb and Cr)
 *   IDCT        jidctint (islow), CONST_BITS 13, PASS1_BITS 2, columns first descaled by 11 bits, then rows by 18, each with round-half-up
 *               ((x + (1 << (n - 1))) >> n); + 128; clamped to 0..255 (saturating, as libjpeg-turbo's SIMD code does)
 *   colour      Cb and Cr are real on ceil(H / 2) x ceil(W / 2); beyond its first and last REAL row a row's neighbour is that row itself.
 *               ceil(W / 2) > 2: h2v2 "fancy" upsampling, s[x] = 3 c[r][x] + c[neighbour row][x] (the row above for output row 2r, below
 *               for 2r + 1), out[2x] = (3 s[x] + s[x-1] + 8) >> 4, out[2x+1] = (3 s[x] + s[x+1] + 7) >> 4, s[-1] := s[0], s[wd] := s[wd-1].
 *               ceil(W / 2) <= 2: 2 x 2 replication.  R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
 *               B = Y + ((116130 cb + 32768) >> 16) with cb, cr minus 128, each clamped to 0..255.
 *   greyscale   8 x 8 blocks, edges replicated, samples minus 128 through the encoder's jfdctint and quantiser with the luma divisors,
 *               then dequantise, IDCT, clamp, crop.
 * Mode RGB decodes int16 zigzag blocks from memory: those mm_jpeg_encode left at mm_jpeg_coef_offset of ITS workspace, given as coef
 * (frames may then be NULL; the decoded frames are those of the very files), or, with coef NULL, those of its own pass of the encoder's
 * transform over frames.  params / params_host: the first 128 words of MMJpegDesc.params, the divisors (the rest may follow; it is not
 * read).  out: bytes (n,H,W,3) / (n,H,W), or with as_float fp32 v / 255 in planes (n,3,H,W) / (n,H,W); 4-byte aligned, never the input.
 * The workspace is the caller's, mm_jpeg_roundtrip_query_workspace bytes, 16-byte aligned (mode RGB: the coefficients unless coef is
 * given, and the Y, Cb and Cr sample planes, 1.5 bytes per pixel of whole MCUs; mode L uses none and the query answers 256).
 * Sampling (mode RGB): the file is that of mm_jpeg_modes_encode with the same sampling, and the sample planes follow its MCU.
 *   4:4:4       no upsampling; convert as above.
 *   4:2:2       Cb and Cr are real on H x ceil(W / 2).  ceil(W / 2) > 2: h2v1 "fancy" upsampling, out[2x] = (3 s[x] + s[x-1] + 1) >> 2,
 *               out[2x+1] = (3 s[x] + s[x+1] + 2) >> 2, s[-1] := s[0], s[wd] := s[wd-1]; otherwise replication.  No vertical neighbour.
 * Return codes as mm_jpeg_encode's: MM_ERR_BAD_SHAPE also for an unknown mode or sampling and for a sampling other than 0 with mode L;
 * MM_ERR_WORKSPACE also for a misaligned coef or out.
 * Mode RGB: two or three launches (transform unless coef is given, idct, pixels); mode L: one.  No host synchronisation; bitwise reproducible.
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_JPEG_MODE_RGB 0
#define MM_JPEG_MODE_L 1
typedef struct MMJpegRoundtripDesc {
    int32_t n, H, W;                /* the frames */
    int32_t mode;                   /* MM_JPEG_MODE_RGB or MM_JPEG_MODE_L */
    int32_t as_float;               /* fp32 planes instead of bytes */
    int32_t sampling;               /* mode RGB: MM_JPEG_SAMPLING_* (0: 4:2:0, as every caller before it had a meaning); mode L: 0 */
    const uint8_t* frames;          /* (n,H,W,3) or (n,H,W), dense, any alignment */
    const int16_t* coef;            /* mode RGB: NULL, or (n, blocks, 64) as mm_jpeg_encode / mm_jpeg_modes_encode of the same sampling leaves them; 16-byte aligned */
    const int32_t* params_host;     /* host memory */
    const int32_t* params;          /* device memory, the same words */
    void* out;
    void* workspace;
    size_t workspace_bytes;
} MMJpegRoundtripDesc;
size_t mm_jpeg_coef_offset(const MMJpegDesc* desc);         /* where the coefficients lie in mm_jpeg_encode's workspace */
size_t mm_jpeg_roundtrip_query_workspace(const MMJpegRoundtripDesc* desc);      /* reads n, H, W, mode and whether coef is NULL */
int mm_jpeg_roundtrip(const MMJpegRoundtripDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * GIF: n device frames (n,H,W,3) of bytes -- what mm_export_grid, mm_export_images, mm_composite_frames and mm_pyramid_frames write, at
 * any byte alignment -- as ONE animated GIF89a file with one global palette of 256 colours.  The file is fully specified here (no other
 * writer's bytes are a target).  Integer arithmetic only; every atomic is an integer one, so their order cannot matter:
 *   histogram  over all frames: bin = (r>>3)<<10 | (g>>3)<<5 | (b>>3), 32768 bins, each a pixel count and the sums of r&7, g&7, b&7
 *   palette    median cut over the non-empty bins.  Box 0 holds them all.  While there are fewer than 256 boxes and some box has at least
 *              two non-empty bins: split the box with the largest pixel count among those (ties: the lowest index) along the axis with
 *              the largest max - min bin coordinate over its non-empty bins (ties: g, then r, then b) at k, the smallest coordinate in
 *              [min, max-1] whose cumulative marginal count from min reaches (count+1)/2 (max-1 if none does).  Bins with coordinate <= k
 *              keep the box's index, the others get index = the number of boxes so far.  Entry i, per channel: (2 s + c) / (2 c) with
 *              c = sum count and s = sum (count * (coord << 3) + low_sum) over the box's bins in 64 bits; unused entries are 0,0,0.
 *   indices    a pixel's index is the box of its bin (the per-bin box array is the lookup table)
 *   LZW        a frame's indices in raster order, cut into segments of `segment` pixels (the last may be shorter) that code
 *              independently.  The frame's stream opens with Clear (256) at 9 bits.  Each segment codes greedily, longest match, with a
 *              fresh dictionary: next = 258, width = 9.  When a new entry receives code next: if next == 1 << width and width < 12 the
 *              width grows by one; then next += 1.  After the segment's last data code the same test is applied once more; then Clear at
 *              that width, or EOI (257) after the frame's last segment.  Codes are packed LSB first; the frame's last byte is zero-padded.
 *   file       "GIF89a"; W, H (u16le), 0xF7, 0, 0; the 768 palette bytes; with loop >= 0: 21 FF 0B "NETSCAPE2.0" 03 01 <loop u16le> 00;
 *              per frame 21 F9 04 04 <delay u16le> 00 00, 2C 0 0 0 0 <W> <H> 00, 08, the stream in sub-blocks of up to 255 bytes each
 *              behind its length byte, 00; finally 3B.
 * palette (768 bytes) and indices (n*H*W bytes) are the caller's device arrays and are always written; with quantize_only nothing else is.
 * The workspace is the caller's, mm_gif_query_workspace bytes, 16-byte aligned; the library allocates nothing.  After the call it holds at
 * byte 0 the file's length as int64 and from byte mm_gif_file_offset on the file: a caller copies the length, then exactly that many
 * bytes.  The rest is scratch: the histogram, the frames' packed streams and a slot per segment sized for its exact worst case (every
 * code new: code k of a segment takes 9 + (k >= 255) + (k >= 767) + (k >= 1791) bits).
 * MM_ERR_BAD_SHAPE: n, H, W < 1; segment outside 1..MM_GIF_MAX_SEGMENT; delay outside 0..65535; loop outside -1..65535.
 * MM_ERR_UNSUPPORTED: H, W or n > 65535; n*H*W >= 2^29 (the queries return 0).  MM_ERR_WORKSPACE: too small or misaligned.
 * Nine stream operations (one memset, eight launches); with quantize_only four (one memset, three launches).  No host synchronisation;
 * bitwise reproducible.
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_GIF_SEGMENT 1024         /* the segment length the Python layer uses */
#define MM_GIF_MAX_SEGMENT 3838     /* 257 + 3838 = 4095: a segment's dictionary can never fill */
typedef struct MMGifDesc {
    int32_t n, H, W;                /* the frames */
    int32_t segment;                /* pixels that share a dictionary */
    int32_t delay;                  /* centiseconds, every frame's unless delays is given */
    int32_t loop;                   /* the NETSCAPE2.0 loop count, or -1 for no such extension */
    int32_t quantize_only;          /* palette and indices only: no file is formed */
    int32_t reserved;               /* 0 */
    const uint8_t* frames;          /* (n,H,W,3), dense, any alignment */
    const int32_t* delays;          /* NULL, or n per-frame delays in device memory (their low 16 bits are used) */
    uint8_t* palette;               /* out: (256,3) */
    uint8_t* indices;               /* out: (n,H,W) */
    void* workspace;
    size_t workspace_bytes;
} MMGifDesc;
size_t mm_gif_query_workspace(const MMGifDesc* desc);       /* reads n, H, W, segment, loop, quantize_only */
size_t mm_gif_file_offset(const MMGifDesc* desc);           /* where the file starts in the workspace */
int mm_gif_encode(const MMGifDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * PNG: n device frames (n,H,W,channels) of bytes, channels 1 (grey), 3 (RGB) or 4 (RGBA) -- what mm_export_images and mm_export_grid
 * write, at any byte alignment -- as n PNG files, back to back.  Lossless: a decoder returns the frames to the bit.  The file is fully
 * specified here (no other writer's bytes are a target).  Integer arithmetic only; every atomic is an integer OR or XOR:
 *   file       89 50 4E 47 0D 0A 1A 0A; IHDR: W, H (u32be), 8, colour type 0 / 2 / 6, 0, 0, 0; one IDAT; IEND.  A chunk is its data's length
 *              u32be, its type, its data and the CRC-32 of type + data u32be.
 *   filter     the stream S is H rows of 1 + W * channels bytes: the filter type, then the filtered row.  bpp = channels; a is the byte bpp
 *              to the left, b the byte above, c above-left, 0 outside the image, of the raw rows.  0 None, 1 Sub x - a, 2 Up x - b,
 *              3 Average x - (a + b) / 2 (floor), 4 Paeth (p = a + b - c: a if |p-a| <= |p-b| and |p-a| <= |p-c|, else b if
 *              |p-b| <= |p-c|, else c), all mod 256.  filter -1 chooses per row the type with the smallest sum of
 *              (v < 128 ? v : 256 - v) over the filtered bytes, ties to the lowest type; 0..4 forces that type on every row.
 *   zlib       78 01, the deflate blocks, zero bits up to a byte, Adler-32 of S (u32be)
 *   deflate    S is cut into segments of `segment` bytes (the last may be shorter), each one block with the fixed Huffman codes: BFINAL
 *              (1 on the last only), then 1, 0, the symbols, end-of-block.  Blocks follow each other bit by bit.
 *   matching   inside a segment [s, e), greedy: at i with i + 3 <= e, j is the latest position in [s, i) with S[j..j+3) == S[i..i+3) and
 *              L the longest length <= min(258, e - i) with S[j+k] == S[i+k] for k < L (overlap allowed).  With such a j the match
 *              (L, i - j) is emitted and i += L; otherwise the literal S[i] and i += 1.
 *   codes      RFC 1951 3.2.6, fixed: Huffman codes most significant bit first into the LSB-first stream, extra bits least significant first.
 * The workspace is the caller's, mm_png_query_workspace bytes, 16-byte aligned; the library allocates nothing.  After the call it holds at
 * byte 0 the n + 1 int64 offsets of the files (the last is the end of the last file) relative to byte mm_png_files_offset, where the
 * files lie back to back: a caller copies the offsets, then exactly offsets[n] bytes.  The rest is scratch: S, a slot per segment sized for
 * its exact worst case (3 + 9 len + 7 bits: a match never costs more than its bytes as literals) and the frames' packed streams.
 * MM_ERR_BAD_SHAPE: n, H, W < 1; channels not 1, 3 or 4; filter outside -1..4; segment outside 1..MM_PNG_MAX_SEGMENT.
 * MM_ERR_UNSUPPORTED: H, W or n > 65535; a frame whose IDAT could exceed 2^31 - 1 bytes; more than 2^31 - 1 segments in the call (the
 * queries return 0).  MM_ERR_WORKSPACE: too small or misaligned.
 * Eight stream operations (one memset, seven launches).  No host synchronisation; bitwise reproducible.
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_PNG_SEGMENT 1024         /* the segment length the Python layer uses (tools/bench_png.py measured 1024, 2048 and 4096) */
#define MM_PNG_MAX_SEGMENT 8192     /* a segment's bytes and its table of 16-bit positions (2 * segment slots) fit 64 KiB of LDS */
#define MM_PNG_CRC_PIECE 64         /* bytes of an IDAT whose CRC one lane takes */
typedef struct MMPngDesc {
    int32_t n, H, W;                /* the frames */
    int32_t channels;               /* 1, 3 or 4: colour type 0, 2 or 6 */
    int32_t filter;                 /* -1: adaptive; 0..4: that filter type on every row */
    int32_t segment;                /* bytes of S that share a match window */
    const uint8_t* frames;          /* (n,H,W,channels), dense, any alignment */
    void* workspace;
    size_t workspace_bytes;
} MMPngDesc;
size_t mm_png_query_workspace(const MMPngDesc* desc);       /* reads n, H, W, channels, segment */
size_t mm_png_files_offset(const MMPngDesc* desc);          /* where the files start in the workspace */
int mm_png_encode(const MMPngDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * FID around the Inception network (csrc/mm_fid.hip; fid_score.py:71-255, inception.py:129-163).  The network stays the caller's.
 *
 * mm_fid_input: 8-bit frames to the network's input batch, one launch, no workspace: out[f, c, y, x] from frames[f, :, :, c] as
 *   t(b) = float(b) / 255.0f (IEEE), h(r) = w0x * t(r, i0x) + w1x * t(r, i1x) on the source rows r = i0y and i1y, v = w0y * h(i0y) + w1y * h(i1y),
 *   out = 2 * v - 1 with `normalize`, v without; every product and sum rounded in fp32, nothing contracted.  The rows {i0, i1, w0, w1} of the
 *   two axes are torch's bilinear resize with align_corners=False lowered by the caller (a single tap is w1 = 0 and i1 = i0 or the clamped
 *   neighbour; no resize is i0 = i1 = the index, w0 = 1, w1 = 0).  params_host is read before the call returns: every index is held to its axis.
 *   MM_ERR_BAD_SHAPE: n < 1; H, W, Ho or Wo outside 1..MM_FID_MAX_SIDE; an index outside its axis.  MM_ERR_UNSUPPORTED: more than 2^31 - 1
 *   workgroups (n * ceil(Ho / 8)).  No host synchronisation; every output float is written by one lane (bitwise reproducible).
 *
 * mm_fid_stats: mu (D) and sigma (D,D) in float64 of N rows of fp32 features, with the meaning of np.mean(act, 0) and
 *   np.cov(act, rowvar=False) of their float64 copy: the data is centred by mu first and the Gram matrix divided once by N - 1.
 *   Order: column sums in float64 over chunks of MM_FID_SUM_ROWS rows, rows ascending, the chunks then added ascending, mu = sum / N; the
 *   centred Gram matrix over splits of MM_FID_SPLIT rows, four rows per v_mfma_f64_16x16x4_f64 step, rows ascending, for the 64 x 64 tiles on or
 *   above the diagonal; the splits added ascending, one division, and (i, j) and (j, i) stored from the same value.  Rows beyond N and columns
 *   beyond D enter as zeros.  No floating-point atomics; bitwise reproducible; sigma is exactly symmetric.  Four launches.
 *   The workspace is the caller's, mm_fid_stats_query_workspace bytes, 256-byte aligned; its contents mean nothing after the call.
 *   MM_ERR_BAD_SHAPE: N < 2 or D < 1.  MM_ERR_UNSUPPORTED: D > 65535 or N > 65535 * MM_FID_SUM_ROWS (the query returns 0).
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_FID_MAX_SIDE 1024        /* H, W, Ho, Wo: sixteen source rows of 3 W bytes fit the default 64 KiB of LDS */
#define MM_FID_SUM_ROWS 256         /* rows of one column-sum chunk */
#define MM_FID_SPLIT 4096           /* rows of one split of the Gram matrix: D = 2048 has 528 tiles, more than two per CU, in every split */
typedef struct MMFidInputDesc {
    int32_t n, H, W;                /* the frames */
    int32_t Ho, Wo;                 /* the output planes */
    int32_t normalize;              /* 1: 2 v - 1 */
    const uint8_t* frames;          /* (n,H,W,3), dense, any alignment */
    const int32_t* params_host;     /* (Wo + Ho, 4) int32 {i0, i1, w0, w1 (float bits)}: the rows of x, then of y */
    const int32_t* params;          /* the same on the device, 16-byte aligned */
    float* out;                     /* (n,3,Ho,Wo), dense; 16-byte stores where it is 16-byte aligned */
} MMFidInputDesc;
int mm_fid_input(const MMFidInputDesc* desc, mm_stream_t stream);

typedef struct MMFidStatsDesc {
    int32_t N, D;                   /* rows and columns of the features */
    const float* x;                 /* (N,D), dense */
    double* mu;                     /* (D) */
    double* sigma;                  /* (D,D) */
    void* workspace;
    size_t workspace_bytes;
} MMFidStatsDesc;
size_t mm_fid_stats_query_workspace(const MMFidStatsDesc* desc);      /* reads N, D */
int mm_fid_stats(const MMFidStatsDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * JPEG decoding: n baseline JPEG FILES, back to back in device memory, as 8-bit frames -- to the byte what Pillow's
 * Image.open(file).convert('RGB') gives (mode RGB; a greyscale file replicates its plane) or .convert('L') of a greyscale file (mode L).
 * csrc/mm_jpeg_decode.hip; the caller parses the markers (jpeg_decode.py: lower_jpeg_decode) and hands over tables of int32 words:
 *   files     n x MM_JPEG_DEC_FILE_INTS: H, W, layout (0: 4:2:0, 1: 4:2:2, 2: 4:4:4, 3: one component), MCU columns, MCU rows, first block,
 *             byte offset of its luma plane, byte offset of its chroma planes, quantisation table of components 0, 1, 2; the rest 0.
 *             Blocks and planes are dense in file order: an MCU has 6, 4, 3 or 1 blocks; the luma plane is MCU rows x MCU columns of
 *             16 x 16, 16 x 8 (wide x high), 8 x 8 or 8 x 8 bytes, the two chroma planes 8 x 8 bytes per MCU each (none for layout 3).
 *   offsets   (n + 1) int64 (8-byte aligned in the table): file i's pixels start at pixel offsets[i] of out, H * W pixels, no padding
 *   segments  n_segments x MM_JPEG_DEC_SEGMENT_INTS: file, first MCU, MCU count, byte begin, byte end, table set.  One lane decodes one
 *             segment; n_segments is a multiple of MM_JPEG_DEC_GROUP and the MM_JPEG_DEC_GROUP segments of a workgroup share one table set
 *             (count 0: a filler).
 *   qtables   n_qtables x 64, natural order, each 1..255
 *   htables   n_htables x MM_JPEG_TABLE_WORDS = 356 words (csrc/mm_jpeg_entropy.h: look-ahead, maxcode, valoffset, symbols)
 *   sets      n_sets x MM_JPEG_DEC_SET_INTS: the tables DC 0, DC 1, AC 0, AC 1; bits 2c / 2c + 1: component c's DC / AC table; the rest 0
 * in this order in one buffer, given twice: tables_host is read (and every record re-checked) before the call returns, tables is the
 * same on the device.  One memset and three launches whatever n: entropy decode (Huffman, FF 00 stuffing, DC prediction per segment) into
 * zeroed int16 zigzag blocks, dequantise + islow IDCT into sample planes, fancy upsampling + YCbCr -> RGB + store (the arithmetic of
 * mm_jpeg_roundtrip).  out may start at any byte.  A damaged stream cannot read or write out of range; its file's status gets
 * MM_JPEG_ST_* bits (csrc/mm_jpeg_entropy.h) and the coefficients after the damage stay zero.
 * The workspace is the caller's, mm_jpeg_decode_query_workspace bytes, 16-byte aligned: the coefficients (128 bytes per block), then, on
 * the next multiple of 256, status (n int32), then the sample planes.
 * MM_ERR_BAD_SHAPE: a count < 1 (n_segments not a positive multiple of MM_JPEG_DEC_GROUP), an unknown mode, a record that contradicts itself or its
 * neighbours (sizes, MCU counts, block or plane or pixel offsets not the running sums, a segment's MCU range outside its file or its
 * bytes outside [0, n_bytes) or not begin <= end, a table index out of range, mixed table sets in a workgroup, a layout other than 3 in
 * mode L, a quantiser outside 1..255).  MM_ERR_UNSUPPORTED: n > MM_JPEG_DEC_MAX_FILES, a file of more than MM_JPEG_MAX_BLOCKS blocks, more
 * than MM_JPEG_DEC_MAX_BLOCKS blocks in the call, n_bytes >= 2^31 (the query returns 0 for all of these).  MM_ERR_WORKSPACE: too small or misaligned, or tables not 16-byte aligned.  Every refusal comes before any GPU work.
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_JPEG_DEC_FILE_INTS 16
#define MM_JPEG_DEC_SEGMENT_INTS 6
#define MM_JPEG_DEC_SET_INTS 8
#define MM_JPEG_DEC_GROUP 16        /* segments of one workgroup (one wave; the other lanes only help to stage the tables): decoding is bound by
                                     * the latency of one lane, so few lanes a wave spread a batch over more CUs and wait for fewer stragglers */
#define MM_JPEG_DEC_MAX_FILES (1 << 20)
#define MM_JPEG_DEC_MAX_BLOCKS (1 << 24)
typedef struct MMJpegDecodeDesc {
    int32_t n;                      /* files */
    int32_t mode;                   /* MM_JPEG_MODE_RGB: out is 3 bytes a pixel; MM_JPEG_MODE_L: 1, greyscale files only */
    int32_t n_segments, n_qtables, n_htables, n_sets;
    int64_t n_bytes;                /* of `bytes` */
    const uint8_t* bytes;           /* the files, back to back; any alignment */
    const int32_t* tables_host;     /* files | offsets | segments | qtables | htables | sets */
    const int32_t* tables;          /* the same on the device, 16-byte aligned */
    uint8_t* out;                   /* offsets[n] * (3 or 1) bytes, any alignment */
    void* workspace;
    size_t workspace_bytes;
} MMJpegDecodeDesc;
size_t mm_jpeg_decode_query_workspace(const MMJpegDecodeDesc* desc);      /* reads the counts and tables_host */
int mm_jpeg_decode(const MMJpegDecodeDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * PNG decoding: n PNG FILES' IDAT data, back to back in device memory, as 8-bit frames -- to the byte what Pillow's
 * Image.open(file).convert(mode) gives for mode L (channels 1), RGB (3) or RGBA (4).  csrc/mm_png_decode.hip; the caller walks the
 * chunks, checks their CRCs and the zlib header (png_decode.py: lower_png_decode) and hands over tables of int32 words:
 *   files     n x MM_PNG_DEC_FILE_INTS: H, W, colour type (0, 2, 3, 4, 6), bit depth (8; 1, 2, 4 for types 0 and 3), bpp (the filters'
 *             distance: 1 below 8 bits, else the file's channels), row_bytes (ceil(W * channels * depth / 8), without the filter byte),
 *             conversion table (types 0 and 3; -1 for the others), byte begin and byte end of the file's raw deflate stream in `bytes`
 *             (its concatenated IDAT data behind the two zlib header bytes), byte offset of its inflated stream S in the workspace
 *             (H * (1 + row_bytes) bytes, dense in file order); the rest 0
 *   offsets   (n + 1) int64 (8-byte aligned in the table): file i's pixels start at pixel offsets[i] of out, H * W pixels, no padding
 *   conv      n_tables x 256 words: for a sample or palette index v the output pixel, channel c in byte c (mode L: byte 0)
 * in this order in one buffer, given twice: tables_host is read (and every record re-checked) before the call returns, tables is the
 * same on the device.  One memset and three launches whatever n: inflate (one wave per file; csrc/mm_inflate.h) into the zeroed S,
 * unfilter in place (filters 0-4), unpack + convert + store.  out may start at any byte.  A damaged stream cannot read or write out of
 * range or spin; its file's status gets MM_PNG_ST_* bits, the bytes of S it did not produce stay zero and the other passes still run.
 * The workspace is the caller's, mm_png_decode_query_workspace bytes, 16-byte aligned: the streams S, then, on the next multiple of
 * 256, status (n int32).
 * MM_ERR_BAD_SHAPE: a count < 1, channels not 1 / 3 / 4, post outside 0..3 or MM_PNG_POST_ALPHA without channels 4, a record that contradicts itself or its neighbours (a size below 1, an unknown
 * colour type, a depth the type does not allow, bpp or row_bytes not what the type, depth and W give, a table index out of range or
 * not -1 where there is none, bytes outside [0, n_bytes] or not begin <= end, stream or pixel offsets not the running sums).
 * MM_ERR_UNSUPPORTED: 16-bit depth, H or W above 65535, n > MM_PNG_DEC_MAX_FILES, n_bytes or the streams above MM_PNG_DEC_MAX_BYTES, more than
 * MM_PNG_DEC_MAX_PIXELS pixels (the query returns 0 for all of these).  MM_ERR_WORKSPACE: too small or misaligned, or tables not 16-byte
 * aligned.  Every refusal comes before any GPU work.
 * ------------------------------------------------------------------------------------------------------------------ */
#define MM_PNG_DEC_FILE_INTS 16
#define MM_PNG_DEC_MAX_FILES (1 << 20)
#define MM_PNG_DEC_MAX_BYTES (1 << 30)
#define MM_PNG_DEC_MAX_PIXELS (1LL << 36)
#define MM_PNG_POST_THRESHOLD 1     /* every output byte that is not 0 becomes 255 (datasets/market.py's seg_loader: point(lambda p: p > 0 and 255)) */
#define MM_PNG_POST_ALPHA 2         /* channels 4 only: out gets the alpha plane alone, one byte a pixel (datasets/thuman2.py's seg_loader) */
#define MM_PNG_ST_OVERRUN 1         /* bits wanted past the stream's end: the reader supplied zeros and the decode stopped at that symbol */
#define MM_PNG_ST_BAD_BLOCK 2       /* BTYPE 3, or a stored block whose LEN and NLEN disagree */
#define MM_PNG_ST_BAD_TABLE 4       /* a dynamic header zlib refuses */
#define MM_PNG_ST_BAD_CODE 8        /* bits that match no code, literal/length symbols 286 / 287, distance symbols 30 / 31 */
#define MM_PNG_ST_BAD_DISTANCE 16   /* a distance that reaches before the first byte produced */
#define MM_PNG_ST_SHORT 32          /* the final block ends before S bytes */
#define MM_PNG_ST_BAD_FILTER 64     /* a filter byte above 4: the row is taken as filter 0 */
typedef struct MMPngDecodeDesc {
    int32_t n;                      /* files */
    int32_t channels;               /* of out: 1 (L), 3 (RGB), 4 (RGBA) */
    int32_t n_tables;               /* conversion tables (0 if no file is grey or palette) */
    int32_t post;                   /* MM_PNG_POST_* bits, 0: the pixels as they are */
    int64_t n_bytes;                /* of `bytes` */
    const uint8_t* bytes;           /* the files' deflate streams, back to back; any alignment */
    const int32_t* tables_host;     /* files | offsets | conv */
    const int32_t* tables;          /* the same on the device, 16-byte aligned */
    uint8_t* out;                   /* offsets[n] * channels bytes (offsets[n] with MM_PNG_POST_ALPHA), any alignment */
    void* workspace;
    size_t workspace_bytes;
} MMPngDecodeDesc;
size_t mm_png_decode_query_workspace(const MMPngDecodeDesc* desc);      /* reads the counts and tables_host */
int mm_png_decode(const MMPngDecodeDesc* desc, mm_stream_t stream);

/* --------------------------------------------------------------------------------------------------------------------
 * Host helpers (no GPU involved)
 * ------------------------------------------------------------------------------------------------------------------ */
/* Build the vertex -> corner CSR from HOST faces (F,3).  offsets: (V+1), items: (3F).  Returns MM_OK or an error. */
int mm_build_vertex_corner_csr(int32_t V, int32_t F, const int32_t* faces_host, int32_t* offsets_host, int32_t* items_host);
/* The same CSR built ON THE DEVICE from device-resident faces, enqueued on the stream (one small launch, no host round trip): what the
 * kaolin-shaped prepare_vertices needs when `faces` arrives as a fresh device tensor on every call (networks.py:272 re-uploads it).
 * offsets_dev (V+1), items_dev (3F), every vertex's list ascending like the host builder's.  Vertex ids outside [0, V) are counted into
 * *status_flag (optional; device or pinned host memory, added to) and left out of the lists.  V <= 12288. */
int mm_build_vertex_corner_csr_device(int32_t V, int32_t F, const int32_t* faces_dev, int32_t* offsets_dev, int32_t* items_dev,
                                      int32_t* status_flag, mm_stream_t stream);
/* The same adjacency with a fixed stride, as MMRenderDesc.vc_table wants it (one trip to memory for a vertex's corners AND their faces'
 * vertex ids, where the CSR needs three).  Returns the stride (the template's largest valence) if table_host is NULL; otherwise fills
 * table_host (V, stride, 4) for the given stride (>= that valence) and returns MM_OK, or an MMStatus error. */
int mm_build_vertex_corner_table(int32_t V, int32_t F, const int32_t* faces_host, int32_t stride, int32_t* table_host);
const char* mm_status_string(int status);
/* After MM_ERR_LAUNCH on this host thread: "<kernel>: <hipGetErrorString> (hipError n)"; "" if none was recorded. */
const char* mm_last_error_detail(void);
/* Layout guard for bindings that mirror the structs by hand (ctypes, cgo, JNI): sizeof of struct #which as the library was
 * compiled, 0 for an unknown id.  Ids: 0 MMRenderDesc, 1 MMRenderGrads, 2 MMReconDesc, 3 MMMeshRegDesc, 4 MMMeshRegGrads,
 * 5 MMAttLossDesc, 6 MMAttLossGrads, 7 MMTexFlowDesc, 8 MMTexFlowGrads, 9 MMPrepareDesc, 10 MMPrepareGrads, 11 MMDibrDesc,
 * 12 MMDibrGrads, 13 MMTexMapDesc, 14 MMTexMapGrads, 15 MMShDesc, 16 MMShGrads, 17 MMMaskIouDesc, 18 MMSsimDesc,
 * 19 MMSsimGrads, 20 MMShapeFeatDesc, 21 MMShapeFeatGrads, 22 MMCameraFeatDesc, 23 MMCameraFeatGrads, 24 MMInterpDesc,
 * 25 MMInterpGrads, 26 MMRenderViewsDesc, 27 MMCriticDesc, 28 MMCriticGrads,
 * 29 MMExportDesc, 30 MMBatchDesc, 32 MMCompositeDesc, 33 MMRenderIndexedDesc, 35 MMPyramidDesc, 37 MMJpegDesc,
 * 38 MMJpegRoundtripDesc, 39 MMGifDesc, 40 MMPoissonDesc, 41 MMPngDesc, 42 MMJpegModesDesc,
 * 43 MMFidInputDesc, 44 MMFidStatsDesc, 45 MMJpegDecodeDesc, 46 MMPngDecodeDesc, 47 MMDisentangleInputsDesc,
 * 48 MMDisentangleDesc, 49 MMDisentangleGrads (31, 34 and 36 are unassigned). */
size_t mm_struct_size(int which);
/* Bumped whenever a struct or the meaning of a field changes (2: op boundary added, reserved uv-tile fields and profiling slot
 * MM_PROF_BIN removed, options bits defined; 3: MMRenderDesc takes the fixed-stride vertex -> corner table instead of the CSR,
 * MM_OPT_BBOX_MIN_CLOSED_MAX_OPEN; 4: MMRenderDesc.geometry_only / status_flag, MMPrepareDesc.proj_device, MMTexMapGrads.workspace, mm_chamfer_nearest, mm_build_vertex_corner_csr_device; 5: MMRenderDesc.fused_contour; 6: MMRenderDesc.fused_totals, mm_recon_data_totals; still 6: the hint bit MM_OPT_MANY_IN_FLIGHT, which changes no result and no layout; 7: MMSsimDesc, MMSsimGrads,
 * mm_ssim_query_workspace / mm_ssim_forward / mm_ssim_backward, struct ids 18 and 19; 8: mm_chamfer_backward, and mm_nearest_neighbour
 * refuses B > 65535 as mm_chamfer_nearest does; 9: MMShapeFeatDesc / Grads, MMCameraFeatDesc / Grads, mm_shape_features_* and
 * mm_camera_features_*, struct ids 20-23; still 9: MMInterpDesc / Grads, mm_interp_query_workspace, mm_collapse_resample and
 * mm_attribute_mix_*, struct ids 24 and 25, which only add -- no existing struct, field or meaning changes; a binding detects them by
 * mm_struct_size(24) != 0; still 9: MMRenderViewsDesc and mm_render_views_*, struct id 26, additions again -- MMRenderDesc and
 * MMRenderGrads keep their layout and meaning; still 9: MMCriticDesc / Grads and mm_critic_inputs_forward / _backward, struct ids 27 and 28,
 * additions once more; a binding detects them by mm_struct_size(27) != 0; still 9: MMExportDesc and mm_export_images / mm_export_grid,
 * struct id 29, an addition too, detected by mm_struct_size(29) != 0; still 9: MMRenderDesc.step_grads, appended behind fused_totals -- no
 * existing field moves or changes meaning and NULL is the old behaviour; the struct grows by one pointer, which a binding built against the
 * shorter struct finds out from mm_struct_size(0), as every binding must check; still 9: MMBatchDesc and mm_assemble_batch, struct id 30, an
 * addition, detected by mm_struct_size(30) != 0; still 9: MMCompositeDesc and mm_composite_frames, struct id 32 -- id 31 stays unassigned and
 * returns 0 --, an addition, detected by mm_struct_size(32) != 0; still 9: MMRenderIndexedDesc and mm_render_indexed_*, struct id 33, an
 * addition, detected by mm_struct_size(33) != 0; still 9: MMPyramidDesc and mm_pyramid_frames, struct id 35 -- id 34 stays unassigned and
 * returns 0 --, an addition, detected by mm_struct_size(35) != 0; still 9: MMJpegDesc and mm_jpeg_*, struct id 37 -- id 36 stays
 * unassigned and returns 0 --, an addition, detected by mm_struct_size(37) != 0; still 9: MMJpegRoundtripDesc,
 * mm_jpeg_roundtrip_query_workspace / mm_jpeg_roundtrip and mm_jpeg_coef_offset, struct id 38, an addition, detected by mm_struct_size(38) != 0; still 9: MMGifDesc and mm_gif_*, struct id 39, an addition, detected by mm_struct_size(39) != 0; still 9: MMPoissonDesc and
 * mm_poisson_frames, struct id 40, an addition, detected by mm_struct_size(40) != 0; still 9: MMPngDesc and mm_png_*, struct id 41, an
 * addition, detected by mm_struct_size(41) != 0; still 9: MMJpegModesDesc and mm_jpeg_modes_*, struct id 42, an addition, detected by
 * mm_struct_size(42) != 0, and MMJpegRoundtripDesc.reserved named sampling, where 0, all a caller could pass, keeps its meaning; still 9: MMFidInputDesc with
 * mm_fid_input, struct id 43, and MMFidStatsDesc with mm_fid_stats_query_workspace / mm_fid_stats, struct id 44, additions, detected by
 * mm_struct_size(43) != 0; still 9: MMJpegDecodeDesc with mm_jpeg_decode_query_workspace / mm_jpeg_decode, struct id 45, an addition, detected by
 * mm_struct_size(45) != 0; still 9: MMPngDecodeDesc with mm_png_decode_query_workspace / mm_png_decode, struct id 46, an addition, detected by
 * mm_struct_size(46) != 0; still 9: the tuning bit MM_OPT_ORDER_LAUNCH, which changes no result and no layout; still 9: MMDisentangleInputsDesc with
 * mm_disentangle_inputs, struct id 47, and MMDisentangleDesc / Grads with mm_disentangle_query_workspace / _forward / _backward, struct ids 48 and 49,
 * additions, detected by mm_struct_size(47) != 0).  Bindings must refuse a library whose version differs from what they mirror. */
#define MM_ABI_VERSION 9
int mm_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MM_RENDER_H */
