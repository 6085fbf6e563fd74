"""ctypes binding of the C ABI in include/mm_render.h (lib/libmm_render.so).

The product path has NO fallback: if the shared library cannot be loaded, or a call returns a negative MMStatus, a
RuntimeError is raised.  torch is used here only for device memory and the current HIP stream.
"""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmm_render.so")
_LIB = None

c_f = ctypes.c_float
c_i = ctypes.c_int32
c_p = ctypes.c_void_p


class MMRenderDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("H", c_i), ("W", c_i), ("V", c_i), ("F", c_i), ("Ht", c_i), ("Wt", c_i), ("no_mask", c_i),
                ("knum", c_i), ("proj", c_f * 3), ("sigmainv", c_f), ("boxlen", c_f), ("multiplier", c_f), ("eps", c_f),
                ("faces", c_p), ("face_uvs", c_p), ("vc_table", c_p), ("vc_stride", c_i),
                ("vertices", c_p), ("textures", c_p), ("lights", c_p), ("bg", c_p), ("azimuths", c_p), ("elevations", c_p),
                ("distances", c_p), ("biases", c_p),
                ("rgba", c_p), ("face_idx", c_p), ("face_normals", c_p), ("imnormal", c_p),
                ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t), ("prof_events", c_p),
                ("fused_gt", c_p), ("fused_image_weight", c_f), ("fused_loss", c_p), ("fused_grad_loss", c_p),
                ("options", c_i), ("geometry_only", c_i), ("status_flag", c_p), ("fused_contour", c_f), ("fused_totals", c_p), ("step_grads", c_p)]


class MMRenderGrads(ctypes.Structure):
    _fields_ = [("grad_rgba", c_p), ("grad_face_normals", c_p), ("grad_vertices", c_p), ("grad_textures", c_p),
                ("grad_lights", c_p), ("grad_bg", c_p), ("grad_azimuths", c_p), ("grad_elevations", c_p),
                ("grad_distances", c_p), ("grad_biases", c_p)]


class MMRenderViewsDesc(ctypes.Structure):
    _fields_ = [("render", MMRenderDesc), ("views", c_i)]


class MMRenderIndexedDesc(ctypes.Structure):
    _fields_ = [("render", MMRenderDesc), ("rows", c_i * 4), ("index", c_p * 4), ("backward", c_i), ("status_flag", c_p)]


class MMReconDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("H", c_i), ("W", c_i), ("pred", c_p), ("pred_strides", ctypes.c_int64 * 4), ("gt", c_p),
                ("image_weight", c_f), ("contour", c_f), ("loss", c_p), ("grad_loss", c_p), ("grad_pred", c_p),
                ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t), ("prof_events", c_p)]

class MMMeshRegDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("V", c_i), ("F", c_i), ("E", c_i), ("terms", ctypes.c_uint32),
                ("lap_offsets", c_p), ("lap_cols", c_p), ("lap_vals", c_p), ("lapT_offsets", c_p), ("lapT_cols", c_p), ("lapT_vals", c_p),
                ("edges", c_p), ("edge2faces", c_p), ("ve_offsets", c_p), ("ve_items", c_p), ("fe_offsets", c_p), ("fe_items", c_p),
                ("flip_index", c_p), ("flipT_offsets", c_p), ("flipT_items", c_p), ("sign_init", c_p),
                ("vertices", c_p), ("delta_vertices", c_p), ("face_normals", c_p), ("ratio", c_f), ("temp", c_f), ("eps", c_f),
                ("losses", c_p), ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


class MMAttributes(ctypes.Structure):
    _fields_ = [(k, c_p) for k in ("azimuths", "elevations", "distances", "biases", "vertices", "textures", "lights")]


class MMAttLossDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("V", c_i), ("Ht", c_i), ("Wt", c_i), ("l1", c_i), ("pred", MMAttributes), ("target", MMAttributes),
                ("losses", c_p), ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


class MMAttLossGrads(ctypes.Structure):
    _fields_ = [("weights", c_p), ("pred", MMAttributes), ("target", MMAttributes)]


class MMDisentangleInputsDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("C", c_i), ("H", c_i), ("W", c_i), ("nhwc", c_i), ("box", c_i * 4), ("boxes_rows", c_i), ("value", c_f),
                ("x", c_p), ("boxes", c_p), ("out_flip", c_p), ("out_erase", c_p)]


# the fourteen tensors of the disentangle terms, in the order MMDisentangleDesc reads them and MMDisentangleGrads writes their gradients
DISENTANGLE_TENSORS = ("textures", "vertices", "azimuths", "elevations", "distances", "biases", "delta_vertices", "flip_textures", "flip_vertices",
                       "jitter_azimuths", "jitter_elevations", "jitter_distances", "jitter_biases", "jitter_delta_vertices")


class MMDisentangleDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("V", c_i), ("Ht", c_i), ("Wt", c_i)] + [(k, c_p) for k in DISENTANGLE_TENSORS] + \
               [("terms", c_p), ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


class MMDisentangleGrads(ctypes.Structure):
    _fields_ = [("weights", c_p)] + [(k, c_p) for k in DISENTANGLE_TENSORS]


class MMTexFlowDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("C", c_i), ("H", c_i), ("W", c_i), ("Ho", c_i), ("Wo", c_i), ("image", c_p), ("flow", c_p), ("textures", c_p)]


class MMTexFlowGrads(ctypes.Structure):
    _fields_ = [("grad_textures", c_p), ("grad_flow", c_p), ("grad_image", c_p)]


class MMMeshRegGrads(ctypes.Structure):
    _fields_ = [("weights", c_p), ("grad_vertices", c_p), ("grad_delta_vertices", c_p), ("grad_face_normals", c_p)]


class MMPrepareDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("V", c_i), ("F", c_i), ("proj", c_f * 3), ("faces", c_p), ("vc_offsets", c_p), ("vc_items", c_p),
                ("vertices", c_p), ("transform", c_p), ("face_vertices_camera", c_p), ("face_vertices_image", c_p), ("face_normals", c_p),
                ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t), ("proj_device", c_p)]


class MMPrepareGrads(ctypes.Structure):
    _fields_ = [("grad_face_vertices_camera", c_p), ("grad_face_vertices_image", c_p), ("grad_face_normals", c_p),
                ("grad_vertices", c_p), ("grad_transform", c_p)]


class MMDibrDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("H", c_i), ("W", c_i), ("F", c_i), ("D", c_i), ("knum", c_i), ("sigmainv", c_f), ("boxlen", c_f),
                ("multiplier", c_f), ("eps", c_f), ("face_vertices_z", c_p), ("face_vertices_image", c_p), ("face_features", c_p),
                ("face_normals_z", c_p), ("interpolated_features", c_p), ("soft_mask", c_p), ("face_idx", c_p),
                ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t), ("options", c_i)]


class MMDibrGrads(ctypes.Structure):
    _fields_ = [("grad_interpolated_features", c_p), ("grad_soft_mask", c_p), ("grad_face_vertices_image", c_p), ("grad_face_features", c_p)]


class MMTexMapDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("N", c_i), ("C", c_i), ("Ht", c_i), ("Wt", c_i), ("mode", c_i), ("uv", c_p), ("textures", c_p), ("out", c_p)]


class MMTexMapGrads(ctypes.Structure):
    _fields_ = [("grad_out", c_p), ("grad_uv", c_p), ("grad_textures", c_p), ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


class MMShDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("N", c_i), ("normals", c_p), ("lights", c_p), ("out", c_p)]


class MMShGrads(ctypes.Structure):
    _fields_ = [("grad_out", c_p), ("grad_normals", c_p), ("grad_lights", c_p)]


class MMMaskIouDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("N", c_i), ("lhs", c_p), ("rhs", c_p), ("sums", c_p), ("loss", c_p)]


SSIM_MAX_WIN = 31                     # MM_SSIM_MAX_WIN
SSIM_NONNEG = 1                       # MM_SSIM_NONNEG


class MMSsimDesc(ctypes.Structure):
    _fields_ = [("N", c_i), ("C", c_i), ("H", c_i), ("W", c_i), ("x", c_p), ("x_strides", ctypes.c_int64 * 4),
                ("y", c_p), ("y_strides", ctypes.c_int64 * 4), ("win_size", c_i), ("win", c_f * SSIM_MAX_WIN), ("C1", c_f), ("C2", c_f),
                ("flags", c_i), ("ssim", c_p), ("cs", c_p), ("mean_c", c_p), ("mean_all", c_p),
                ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


class MMSsimGrads(ctypes.Structure):
    _fields_ = [("grad_ssim", c_p), ("grad_cs", c_p), ("grad_x", c_p), ("grad_y", c_p)]


ENCFEAT_MAX_V = 14336                 # MM_ENCFEAT_MAX_V
DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2


class MMShapeFeatDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("C", c_i), ("H", c_i), ("W", c_i), ("V", c_i), ("x_dtype", c_i), ("x", c_p),
                ("x_strides", ctypes.c_int64 * 4), ("template_xyz", c_p), ("col_k", c_i), ("col_idx", c_p), ("col_val", c_p),
                ("row_k", c_i), ("row_idx", c_p), ("row_val", c_p), ("p", c_p), ("out", c_p),
                ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


class MMShapeFeatGrads(ctypes.Structure):
    _fields_ = [("grad_out", c_p), ("grad_x", c_p), ("grad_p", c_p)]


class MMCameraFeatDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("C", c_i), ("H", c_i), ("W", c_i), ("V", c_i), ("x_dtype", c_i), ("x", c_p),
                ("x_strides", ctypes.c_int64 * 4), ("template_xyz", c_p), ("p_map", c_p), ("p_local", c_p), ("out", c_p),
                ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


class MMCameraFeatGrads(ctypes.Structure):
    _fields_ = [("grad_out", c_p), ("grad_x", c_p), ("grad_p_map", c_p), ("grad_p_local", c_p)]


class MMInterpDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("V", c_i), ("Ht", c_i), ("Wt", c_i), ("H", c_i), ("W", c_i),
                ("vertices", c_p), ("delta_vertices", c_p), ("textures", c_p), ("bg", c_p), ("lights", c_p),
                ("out_vertices", c_p), ("out_delta_vertices", c_p), ("out_textures", c_p), ("out_bg", c_p), ("out_lights", c_p),
                ("idx_a", c_p), ("idx_b", c_p), ("alpha_shape", c_p), ("alpha_texture", c_p), ("alpha_light", c_p),
                ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


class MMInterpGrads(ctypes.Structure):
    _fields_ = [("grad_out_vertices", c_p), ("grad_out_delta_vertices", c_p), ("grad_out_textures", c_p), ("grad_out_bg", c_p),
                ("grad_out_lights", c_p), ("grad_vertices", c_p), ("grad_delta_vertices", c_p), ("grad_textures", c_p), ("grad_bg", c_p),
                ("grad_lights", c_p)]


class MMCriticDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("H", c_i), ("W", c_i), ("unmask", c_i), ("Xa", c_p), ("Xer90", c_p), ("Xir", c_p),
                ("Xa_nhwc", c_i), ("Xer90_nhwc", c_i), ("Xir_nhwc", c_i), ("alpha_er90", c_p), ("alpha_ir", c_p),
                ("out_batch", c_p), ("out_gp_er90", c_p), ("out_gp_ir", c_p)]


class MMCriticGrads(ctypes.Structure):
    _fields_ = [("g_batch", c_p), ("grad_er90", c_p), ("grad_ir", c_p), ("grad_er90_nhwc", c_i), ("grad_ir_nhwc", c_i)]


class MMExportDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("N", c_i), ("C", c_i), ("H", c_i), ("W", c_i), ("nhwc", c_i), ("rounding", c_i), ("white", c_i),
                ("as_float", c_i), ("nrow", c_i), ("padding", c_i), ("pad_value", c_f), ("x", c_p), ("out_rgb", c_p), ("out_mask", c_p),
                ("out_rgba", c_p), ("out_grid", c_p)]


class MMBatchDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("H", c_i), ("W", c_i), ("n_images", c_i), ("bg", c_i), ("reserved", c_i), ("images", c_p), ("segs", c_p),
                ("offsets", c_p), ("sizes", c_p), ("records_host", c_p), ("records", c_p), ("out", c_p)]


class MMCompositeDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("H", c_i), ("W", c_i), ("n_fg", c_i), ("n_bg", c_i), ("bg_C", c_i), ("fg_nhwc", c_i), ("fill_holes", c_i),
                ("mask_k", c_i), ("bg_k", c_i), ("mask_pad", c_i), ("bg_pad", c_i * 4), ("rounding", c_i), ("as_float", c_i),
                ("reserved", c_i), ("renders", c_p), ("backgrounds", c_p), ("params_host", c_p), ("params", c_p), ("out", c_p)]


class MMPyramidDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("H", c_i), ("W", c_i), ("n_fg", c_i), ("n_bg", c_i), ("bg_C", c_i), ("fg_nhwc", c_i), ("k", c_i),
                ("bg_pad", c_i * 4), ("rounding", c_i), ("as_float", c_i),
                ("renders", c_p), ("backgrounds", c_p), ("params_host", c_p), ("params", c_p), ("out", c_p)]


POISSON_MAX_SWEEPS = 1 << 16          # MM_POISSON_MAX_SWEEPS


class MMPoissonDesc(ctypes.Structure):
    _fields_ = [("B", c_i), ("H", c_i), ("W", c_i), ("n_fg", c_i), ("n_bg", c_i), ("bg_C", c_i), ("fg_nhwc", c_i), ("border", c_i),
                ("bg_pad", c_i * 4), ("rounding", c_i), ("as_float", c_i), ("sweeps", c_i), ("omega", c_f),
                ("renders", c_p), ("backgrounds", c_p), ("mask", c_p), ("params_host", c_p), ("params", c_p), ("out", c_p)]


class MMJpegDesc(ctypes.Structure):
    _fields_ = [("n", c_i), ("H", c_i), ("W", c_i), ("header_bytes", c_i), ("frames", c_p), ("params_host", c_p), ("params", c_p),
                ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


JPEG_MODE_RGB, JPEG_MODE_L = 0, 1     # MM_JPEG_MODE_*
JPEG_SAMPLING_420, JPEG_SAMPLING_422, JPEG_SAMPLING_444 = 0, 1, 2      # MM_JPEG_SAMPLING_*


class MMJpegModesDesc(ctypes.Structure):
    _fields_ = [("n", c_i), ("H", c_i), ("W", c_i), ("header_bytes", c_i), ("mode", c_i), ("sampling", c_i), ("frames", c_p), ("params_host", c_p),
                ("params", c_p), ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


class MMJpegRoundtripDesc(ctypes.Structure):
    _fields_ = [("n", c_i), ("H", c_i), ("W", c_i), ("mode", c_i), ("as_float", c_i), ("sampling", c_i), ("frames", c_p), ("coef", c_p),
                ("params_host", c_p), ("params", c_p), ("out", c_p), ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


JPEG_DEC_FILE_INTS, JPEG_DEC_SEGMENT_INTS, JPEG_DEC_SET_INTS, JPEG_TABLE_WORDS = 16, 6, 8, 356      # MM_JPEG_DEC_*_INTS, MM_JPEG_TABLE_WORDS
JPEG_DEC_MAX_FILES, JPEG_DEC_MAX_BLOCKS, JPEG_DEC_GROUP = 1 << 20, 1 << 24, 16      # MM_JPEG_DEC_MAX_*, MM_JPEG_DEC_GROUP


class MMJpegDecodeDesc(ctypes.Structure):
    _fields_ = [("n", c_i), ("mode", c_i), ("n_segments", c_i), ("n_qtables", c_i), ("n_htables", c_i), ("n_sets", c_i), ("n_bytes", ctypes.c_int64),
                ("bytes", c_p), ("tables_host", c_p), ("tables", c_p), ("out", c_p), ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


PNG_DEC_FILE_INTS, PNG_DEC_MAX_FILES, PNG_DEC_MAX_BYTES, PNG_DEC_MAX_PIXELS = 16, 1 << 20, 1 << 30, 1 << 36      # MM_PNG_DEC_*
PNG_POST_THRESHOLD, PNG_POST_ALPHA = 1, 2      # MM_PNG_POST_*


class MMPngDecodeDesc(ctypes.Structure):
    _fields_ = [("n", c_i), ("channels", c_i), ("n_tables", c_i), ("post", c_i), ("n_bytes", ctypes.c_int64),
                ("bytes", c_p), ("tables_host", c_p), ("tables", c_p), ("out", c_p), ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


GIF_SEGMENT, GIF_MAX_SEGMENT = 1024, 3838      # MM_GIF_SEGMENT, MM_GIF_MAX_SEGMENT


class MMGifDesc(ctypes.Structure):
    _fields_ = [("n", c_i), ("H", c_i), ("W", c_i), ("segment", c_i), ("delay", c_i), ("loop", c_i), ("quantize_only", c_i), ("reserved", c_i),
                ("frames", c_p), ("delays", c_p), ("palette", c_p), ("indices", c_p), ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


PNG_SEGMENT, PNG_MAX_SEGMENT, PNG_CRC_PIECE = 1024, 8192, 64      # MM_PNG_SEGMENT, MM_PNG_MAX_SEGMENT, MM_PNG_CRC_PIECE


class MMPngDesc(ctypes.Structure):
    _fields_ = [("n", c_i), ("H", c_i), ("W", c_i), ("channels", c_i), ("filter", c_i), ("segment", c_i),
                ("frames", c_p), ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


FID_MAX_SIDE, FID_SUM_ROWS, FID_SPLIT = 1024, 256, 4096      # MM_FID_MAX_SIDE, MM_FID_SUM_ROWS, MM_FID_SPLIT


class MMFidInputDesc(ctypes.Structure):
    _fields_ = [("n", c_i), ("H", c_i), ("W", c_i), ("Ho", c_i), ("Wo", c_i), ("normalize", c_i), ("frames", c_p), ("params_host", c_p),
                ("params", c_p), ("out", c_p)]


class MMFidStatsDesc(ctypes.Structure):
    _fields_ = [("N", c_i), ("D", c_i), ("x", c_p), ("mu", c_p), ("sigma", c_p), ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


PROF_RENDER = ("vertex_fwd", "raster_fwd", "pixel_bwd", "gather_bwd", "vertex_bwd", "order")
ABI_VERSION = 9
OPT_WALK_BLOCK, OPT_WALK_WAVE = 1 << 1, 1 << 2
OPT_CULL_STRICT, OPT_SOFT_SKIP_CULLED, OPT_BBOX_HALF_OPEN, OPT_BARY_ONE_MINUS, OPT_SH_ORDER_XYZ = 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 8
OPT_BBOX_MIN_CLOSED_MAX_OPEN = 1 << 9
OPT_WALK_QUEUE, OPT_WALK_BATCH = 1 << 10, 1 << 11
OPT_MANY_IN_FLIGHT = 1 << 12          # hint: several independent calls in flight (identical results; include/mm_render.h)
OPT_ORDER_LAUNCH = 1 << 13            # tuning / tests: the tile sort in a launch of its own, also where the vertex launch would do it (identical results)
PROF_RECON = ("recon_partial", "recon_final", "recon_bwd", "recon_contour")


P, c_z, c_int = ctypes.POINTER, ctypes.c_size_t, ctypes.c_int

# The C ABI of include/mm_render.h, declared once: export name -> (restype, argtypes).  lib() applies it, EXPORTS is its keys, and
# tests/test_abi_and_host.py holds every row against the header.  A stream (mm_stream_t) and a raw array are c_p.
SIGNATURES = {
    "mm_query_workspace": (c_z, [P(MMRenderDesc)]),
    "mm_render_forward": (c_int, [P(MMRenderDesc), c_p]),
    "mm_render_backward": (c_int, [P(MMRenderDesc), P(MMRenderGrads), c_p]),
    "mm_render_status": (c_int, [P(MMRenderDesc), c_p, P(c_i)]),
    "mm_render_fused_loss": (c_int, [P(MMRenderDesc), c_p]),
    "mm_render_step_mode": (c_int, [P(MMRenderDesc)]),
    "mm_debug_step_layout": (c_int, [P(MMRenderDesc), P(c_z)]),
    "mm_debug_workspace_layout": (c_int, [P(MMRenderDesc), P(c_z)]),
    "mm_render_views_query_workspace": (c_z, [P(MMRenderViewsDesc)]),
    "mm_render_views_forward": (c_int, [P(MMRenderViewsDesc), c_p]),
    "mm_render_views_backward": (c_int, [P(MMRenderViewsDesc), P(MMRenderGrads), c_p]),
    "mm_render_indexed_query_workspace": (c_z, [P(MMRenderIndexedDesc)]),
    "mm_render_indexed_forward": (c_int, [P(MMRenderIndexedDesc), c_p]),
    "mm_render_indexed_backward": (c_int, [P(MMRenderIndexedDesc), P(MMRenderGrads), c_p]),
    "mm_recon_query_workspace": (c_z, [P(MMReconDesc)]),
    "mm_recon_data_forward": (c_int, [P(MMReconDesc), c_p]),
    "mm_recon_data_backward": (c_int, [P(MMReconDesc), c_p]),
    "mm_recon_data_totals": (c_p, [P(MMReconDesc)]),
    "mm_nearest_neighbour": (c_int, [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "mm_chamfer_nearest": (c_int, [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "mm_chamfer_backward": (c_int, [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "mm_mesh_reg_query_workspace": (c_z, [P(MMMeshRegDesc)]),
    "mm_mesh_reg_forward": (c_int, [P(MMMeshRegDesc), c_p]),
    "mm_mesh_reg_backward": (c_int, [P(MMMeshRegDesc), P(MMMeshRegGrads), c_p]),
    "mm_attribute_loss_query_workspace": (c_z, [P(MMAttLossDesc)]),
    "mm_attribute_loss_forward": (c_int, [P(MMAttLossDesc), c_p]),
    "mm_attribute_loss_backward": (c_int, [P(MMAttLossDesc), P(MMAttLossGrads), c_p]),
    "mm_disentangle_inputs": (c_int, [P(MMDisentangleInputsDesc), c_p]),
    "mm_disentangle_query_workspace": (c_z, [P(MMDisentangleDesc)]),
    "mm_disentangle_forward": (c_int, [P(MMDisentangleDesc), c_p]),
    "mm_disentangle_backward": (c_int, [P(MMDisentangleDesc), P(MMDisentangleGrads), c_p]),
    "mm_texture_flow_forward": (c_int, [P(MMTexFlowDesc), c_p]),
    "mm_texture_flow_backward": (c_int, [P(MMTexFlowDesc), P(MMTexFlowGrads), c_p]),
    "mm_prepare_vertices_query_workspace": (c_z, [P(MMPrepareDesc)]),
    "mm_prepare_vertices_forward": (c_int, [P(MMPrepareDesc), c_p]),
    "mm_prepare_vertices_backward": (c_int, [P(MMPrepareDesc), P(MMPrepareGrads), c_p]),
    "mm_face_normals_forward": (c_int, [ctypes.c_int64, c_i, c_p, c_p, c_p]),
    "mm_face_normals_backward": (c_int, [ctypes.c_int64, c_i, c_p, c_p, c_p, c_p]),
    "mm_dibr_query_workspace": (c_z, [P(MMDibrDesc)]),
    "mm_dibr_rasterization_forward": (c_int, [P(MMDibrDesc), c_p]),
    "mm_dibr_rasterization_backward": (c_int, [P(MMDibrDesc), P(MMDibrGrads), c_p]),
    "mm_texture_mapping_backward_query_workspace": (c_z, [P(MMTexMapDesc)]),
    "mm_texture_mapping_forward": (c_int, [P(MMTexMapDesc), c_p]),
    "mm_texture_mapping_backward": (c_int, [P(MMTexMapDesc), P(MMTexMapGrads), c_p]),
    "mm_sh_lighting_forward": (c_int, [P(MMShDesc), c_p]),
    "mm_sh_lighting_backward": (c_int, [P(MMShDesc), P(MMShGrads), c_p]),
    "mm_mask_iou_forward": (c_int, [P(MMMaskIouDesc), c_p]),
    "mm_mask_iou_backward": (c_int, [P(MMMaskIouDesc), c_p, c_p, c_p, c_p]),
    "mm_ssim_query_workspace": (c_z, [P(MMSsimDesc)]),
    "mm_ssim_forward": (c_int, [P(MMSsimDesc), c_p]),
    "mm_ssim_backward": (c_int, [P(MMSsimDesc), P(MMSsimGrads), c_p]),
    "mm_shape_features_query_workspace": (c_z, [P(MMShapeFeatDesc)]),
    "mm_shape_features_forward": (c_int, [P(MMShapeFeatDesc), c_p]),
    "mm_shape_features_backward": (c_int, [P(MMShapeFeatDesc), P(MMShapeFeatGrads), c_p]),
    "mm_camera_features_query_workspace": (c_z, [P(MMCameraFeatDesc)]),
    "mm_camera_features_forward": (c_int, [P(MMCameraFeatDesc), c_p]),
    "mm_camera_features_backward": (c_int, [P(MMCameraFeatDesc), P(MMCameraFeatGrads), c_p]),
    "mm_interp_query_workspace": (c_z, [P(MMInterpDesc)]),
    "mm_collapse_resample": (c_int, [c_i, c_i, c_p, c_p, c_p, c_p, c_f, c_p, c_p]),
    "mm_attribute_mix_forward": (c_int, [P(MMInterpDesc), c_p]),
    "mm_attribute_mix_backward": (c_int, [P(MMInterpDesc), P(MMInterpGrads), c_p]),
    "mm_critic_inputs_forward": (c_int, [P(MMCriticDesc), c_p]),
    "mm_critic_inputs_backward": (c_int, [P(MMCriticDesc), P(MMCriticGrads), c_p]),
    "mm_export_images": (c_int, [P(MMExportDesc), c_p]),
    "mm_export_grid": (c_int, [P(MMExportDesc), c_p]),
    "mm_assemble_batch": (c_int, [P(MMBatchDesc), c_p]),
    "mm_composite_frames": (c_int, [P(MMCompositeDesc), c_p]),
    "mm_pyramid_frames": (c_int, [P(MMPyramidDesc), c_p]),
    "mm_poisson_frames": (c_int, [P(MMPoissonDesc), c_p]),
    "mm_jpeg_query_workspace": (c_z, [P(MMJpegDesc)]),
    "mm_jpeg_files_offset": (c_z, [P(MMJpegDesc)]),
    "mm_jpeg_encode": (c_int, [P(MMJpegDesc), c_p]),
    "mm_jpeg_modes_query_workspace": (c_z, [P(MMJpegModesDesc)]),
    "mm_jpeg_modes_files_offset": (c_z, [P(MMJpegModesDesc)]),
    "mm_jpeg_modes_coef_offset": (c_z, [P(MMJpegModesDesc)]),
    "mm_jpeg_modes_encode": (c_int, [P(MMJpegModesDesc), c_p]),
    "mm_jpeg_coef_offset": (c_z, [P(MMJpegDesc)]),
    "mm_jpeg_roundtrip_query_workspace": (c_z, [P(MMJpegRoundtripDesc)]),
    "mm_jpeg_roundtrip": (c_int, [P(MMJpegRoundtripDesc), c_p]),
    "mm_gif_query_workspace": (c_z, [P(MMGifDesc)]),
    "mm_gif_file_offset": (c_z, [P(MMGifDesc)]),
    "mm_gif_encode": (c_int, [P(MMGifDesc), c_p]),
    "mm_png_query_workspace": (c_z, [P(MMPngDesc)]),
    "mm_png_files_offset": (c_z, [P(MMPngDesc)]),
    "mm_png_encode": (c_int, [P(MMPngDesc), c_p]),
    "mm_jpeg_decode_query_workspace": (c_z, [P(MMJpegDecodeDesc)]),
    "mm_jpeg_decode": (c_int, [P(MMJpegDecodeDesc), c_p]),
    "mm_png_decode_query_workspace": (c_z, [P(MMPngDecodeDesc)]),
    "mm_png_decode": (c_int, [P(MMPngDecodeDesc), c_p]),
    "mm_fid_input": (c_int, [P(MMFidInputDesc), c_p]),
    "mm_fid_stats_query_workspace": (c_z, [P(MMFidStatsDesc)]),
    "mm_fid_stats": (c_int, [P(MMFidStatsDesc), c_p]),
    "mm_build_vertex_corner_csr": (c_int, [c_i, c_i, c_p, c_p, c_p]),
    "mm_build_vertex_corner_csr_device": (c_int, [c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    "mm_build_vertex_corner_table": (c_int, [c_i, c_i, c_p, c_i, c_p]),
    "mm_status_string": (ctypes.c_char_p, [c_int]),
    "mm_last_error_detail": (ctypes.c_char_p, []),
    "mm_struct_size": (c_z, [c_int]),
    "mm_abi_version": (c_int, []),
}
EXPORTS = tuple(SIGNATURES)

# mm_struct_size's ids (include/mm_render.h, "Ids:"); 31, 34 and 36 are unassigned
STRUCT_IDS = {0: MMRenderDesc, 1: MMRenderGrads, 2: MMReconDesc, 3: MMMeshRegDesc, 4: MMMeshRegGrads, 5: MMAttLossDesc, 6: MMAttLossGrads,
              7: MMTexFlowDesc, 8: MMTexFlowGrads, 9: MMPrepareDesc, 10: MMPrepareGrads, 11: MMDibrDesc, 12: MMDibrGrads, 13: MMTexMapDesc,
              14: MMTexMapGrads, 15: MMShDesc, 16: MMShGrads, 17: MMMaskIouDesc, 18: MMSsimDesc, 19: MMSsimGrads, 20: MMShapeFeatDesc,
              21: MMShapeFeatGrads, 22: MMCameraFeatDesc, 23: MMCameraFeatGrads, 24: MMInterpDesc, 25: MMInterpGrads, 26: MMRenderViewsDesc,
              27: MMCriticDesc, 28: MMCriticGrads, 29: MMExportDesc, 30: MMBatchDesc, 32: MMCompositeDesc, 33: MMRenderIndexedDesc,
              35: MMPyramidDesc, 37: MMJpegDesc, 38: MMJpegRoundtripDesc, 39: MMGifDesc, 40: MMPoissonDesc, 41: MMPngDesc, 42: MMJpegModesDesc,
              43: MMFidInputDesc, 44: MMFidStatsDesc, 45: MMJpegDecodeDesc, 46: MMPngDecodeDesc, 47: MMDisentangleInputsDesc, 48: MMDisentangleDesc,
              49: MMDisentangleGrads}

_FN = {}          # export name -> bound function, filled by lib()


def lib():
    """Load libmm_render.so (building it in-tree first, under a file lock, if the sources are newer and hipcc is available).
    A failed rebuild raises -- a stale library is never used silently -- and the library's ABI version and struct sizes are
    checked against this binding's mirror of include/mm_render.h."""
    global _LIB
    if _LIB is not None:
        return _LIB
    from . import build_native
    if build_native.needs_build():
        if os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
            try:
                build_native.build()
            except Exception as e:
                raise RuntimeError("libmm_render.so is out of date and rebuilding it failed: %s" % e)
        elif os.path.exists(LIB_PATH):
            raise RuntimeError("libmm_render.so is older than its sources and hipcc is not available to rebuild it")
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libmm_render.so not found at %s (run __graft_entry__.build())" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    fns = {}
    for name, (restype, argtypes) in SIGNATURES.items():
        if not hasattr(L, name):
            raise RuntimeError("libmm_render.so does not export %s" % name)
        f = fns[name] = getattr(L, name)
        f.restype = restype
        f.argtypes = argtypes
    if L.mm_abi_version() != ABI_VERSION:
        raise RuntimeError("libmm_render.so has ABI version %d, this binding mirrors version %d" % (L.mm_abi_version(), ABI_VERSION))
    for i, cls in STRUCT_IDS.items():
        if L.mm_struct_size(i) != ctypes.sizeof(cls):
            raise RuntimeError("struct layout mismatch for %s: library %d bytes, binding %d" % (cls.__name__, L.mm_struct_size(i), ctypes.sizeof(cls)))
    _FN.update(fns)
    _LIB = L
    return L


def check(status, what):
    if status != 0:
        detail = lib().mm_last_error_detail().decode() if status == -4 else ""
        raise RuntimeError("%s failed: %s (MMStatus %d)%s" % (what, lib().mm_status_string(status).decode(), status,
                                                            " [" + detail + "]" if detail else ""))


_EXT = None


def torch_ext():
    """The C++ autograd nodes of the class API (lib/mm_torch_ext.so from csrc/mm_torch_ext.cpp; diff_render.py has no other host path).
    Loaded like lib(): a missing module, or one older than its sources, is built first (build_native.build_torch_ext: host compiler only,
    file lock, atomic publish); a failed build or load, or a module whose MMRenderDesc is not this binding's, raises -- never a stale module."""
    global _EXT
    if _EXT is not None:
        return _EXT
    import importlib.machinery
    import importlib.util
    from . import build_native as bn
    try:
        path = bn.build_torch_ext()
        loader = importlib.machinery.ExtensionFileLoader("mm_torch_ext", path)
        mod = importlib.util.module_from_spec(importlib.util.spec_from_loader("mm_torch_ext", loader))
        loader.exec_module(mod)
    except Exception as e:
        raise RuntimeError("lib/mm_torch_ext.so could not be built or loaded (%s): rebuild it with `python __graft_entry__.py`" % e)
    if mod.desc_bytes() != ctypes.sizeof(MMRenderDesc):
        raise RuntimeError("lib/mm_torch_ext.so was built against an MMRenderDesc of %d bytes, this binding's is %d: rebuild it with "
                           "`python __graft_entry__.py`" % (mod.desc_bytes(), ctypes.sizeof(MMRenderDesc)))
    _EXT = mod
    return mod


_ADDR = {}


def fn_addr(name):
    """address of an exported function of the library, for the C++ autograd nodes (torch_ext)"""
    a = _ADDR.get(name)
    if a is None:
        a = _ADDR[name] = ctypes.cast(getattr(lib(), name), ctypes.c_void_p).value
    return a


def as_f32(t, dev):
    """``t`` detached as a dense fp32 tensor on ``dev``; the common case (already so) costs one attribute test each."""
    if t is None:
        return None
    if t.dtype is torch.float32 and t.device == dev and t.is_contiguous():
        return t.detach()
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def upload_int32(values, device, wait=False):
    """int32 ``values`` (a tensor, or an array that is cast) to ``device`` through pinned host memory, without waiting: (host, dev).  A
    descriptor may name the pinned copy as its host table; it is read before the call returns.

    The copy is queued on the device's current stream, so the device tensor is ordered only against work queued there after it: right for a
    table that one call uploads and the same call's kernels read.  wait=True is for a table that is cached and shared: the host waits for
    that copy (an event behind it, not the whole device), so the table is finished on return and a later call on any stream may read it."""
    src = values if torch.is_tensor(values) else torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32))
    host = torch.empty(src.shape, dtype=torch.int32, pin_memory=True)
    host.copy_(src)
    dev = host.to(device, non_blocking=True)
    if wait and dev.is_cuda:
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev.device))
        done.synchronize()
    return host, dev


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream(device):
    """The current HIP stream of ``device`` as a void* (the raw-handle query when torch offers it: the Stream object costs microseconds)."""
    if _raw_stream is not None and device.index is not None:
        return ctypes.c_void_p(_raw_stream(device.index))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def fn(name):
    """export ``name`` as lib() bound it (restype and argtypes from SIGNATURES); a name the table lacks raises before anything is called"""
    f = _FN.get(name)
    if f is None:
        if name not in SIGNATURES:
            raise RuntimeError("%s is not an export of libmm_render.so (see _native.SIGNATURES)" % name)
        lib()
        f = _FN[name]
    return f


def call(name, where, *args, what=None):
    """Call export ``name`` with ``args`` followed by the stream and raise (check) on a non-zero status, labelled ``what or name``.  ``where`` is a
    torch.device, whose current stream is taken, or a ready c_void_p stream.  A Structure goes in as itself: argtypes passes it by reference.

    The one call path of every entry point that takes a stream and returns an MMStatus.  Deliberately not folded in: input_batches.py turns a
    refusal of mm_assemble_batch into a ValueError of its own wording (it uses fn, not check); mm_render_status returns a verdict, not an
    error; the *_query_workspace functions, mm_jpeg_files_offset, mm_jpeg_coef_offset and their mm_jpeg_modes_* forms, mm_gif_file_offset, mm_recon_data_totals and mm_render_step_mode return values (fn(name)(desc));
    and diff_render.py hands fn_addr addresses to the C++ nodes."""
    status = (_FN.get(name) or fn(name))(*args, where if type(where) is c_p else current_stream(where))
    if status:
        check(status, what or name)


def workspace(query_name, desc, device, zero=False, at_least=0):
    """A uint8 workspace of max(``query_name``(desc), at_least) bytes on ``device``, zero-filled if ``zero``; desc.workspace is set to it and
    desc.workspace_bytes to the queried size.  The caller keeps the returned tensor alive for as long as the descriptor is used."""
    nbytes = fn(query_name)(desc)
    t = (torch.zeros if zero else torch.empty)(max(nbytes, at_least), device=device, dtype=torch.uint8)
    desc.workspace, desc.workspace_bytes = t.data_ptr(), nbytes
    return t


def up256(x):
    """x rounded up to a multiple of 256: where the next array of a workspace starts (align256 in csrc/mm_device.h)"""
    return (x + 255) // 256 * 256


def checked_workspace(query_name, desc, device, want, offset_names, text):
    """``workspace(query_name, desc, device)``, held to the Python mirror of its layout: ``want`` is (bytes, offset, ...), the offsets those
    the exports ``offset_names`` give for desc.  Any difference raises RuntimeError(text(got, want)), both tuples like ``want``."""
    ws = workspace(query_name, desc, device)
    got = (desc.workspace_bytes,) + tuple(fn(name)(desc) for name in offset_names)
    if got != tuple(want):
        raise RuntimeError(text(got, tuple(want)))
    return ws


def read_back(ws, k, at):
    """Files out of a workspace after two blocking copies through pinned host memory: the k int64 words at its head, then exactly
    words[-1] bytes from byte ``at`` on.  (the words as a list, the bytes as a pinned uint8 tensor)"""
    head = torch.empty((k,), dtype=torch.int64, pin_memory=True)
    head.copy_(ws[:8 * k].view(torch.int64))                             # copy 1 (blocking): the lengths
    words = head.tolist()
    buf = torch.empty((words[-1],), dtype=torch.uint8, pin_memory=True)
    buf.copy_(ws[at:at + words[-1]])                                     # copy 2 (blocking): exactly the bytes used
    return words, buf


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("the MI355X render path needs tensors in device memory (got a %s tensor); "
                               "there is no CPU fallback" % t.device)
