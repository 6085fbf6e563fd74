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


class MMJpegDesc(ctypes.Structure):
    _fields_ = [("n", c_i), ("H", c_i), ("W", c_i), ("header_bytes", c_i), ("frames", c_p), ("params_host", c_p), ("params", c_p),
                ("workspace", c_p), ("workspace_bytes", ctypes.c_size_t)]


PROF_RENDER = ("vertex_fwd", "raster_fwd", "pixel_bwd", "gather_bwd", "vertex_bwd", "order")
ABI_VERSION = 9
OPT_WALK_BLOCK, OPT_WALK_WAVE = 1 << 1, 1 << 2
OPT_CULL_STRICT, OPT_SOFT_SKIP_CULLED, OPT_BBOX_HALF_OPEN, OPT_BARY_ONE_MINUS, OPT_SH_ORDER_XYZ = 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 8
OPT_BBOX_MIN_CLOSED_MAX_OPEN = 1 << 9
OPT_WALK_QUEUE, OPT_WALK_BATCH = 1 << 10, 1 << 11
OPT_MANY_IN_FLIGHT = 1 << 12          # hint: several independent calls in flight (identical results; include/mm_render.h)
PROF_RECON = ("recon_partial", "recon_final", "recon_bwd", "recon_contour")

EXPORTS = ("mm_query_workspace", "mm_render_forward", "mm_render_backward", "mm_render_status", "mm_render_fused_loss", "mm_render_step_mode", "mm_debug_step_layout", "mm_debug_workspace_layout", "mm_recon_query_workspace",
           "mm_recon_data_forward", "mm_recon_data_backward", "mm_recon_data_totals", "mm_build_vertex_corner_csr", "mm_build_vertex_corner_csr_device", "mm_build_vertex_corner_table", "mm_nearest_neighbour", "mm_chamfer_nearest", "mm_chamfer_backward", "mm_status_string", "mm_last_error_detail",
           "mm_mesh_reg_query_workspace", "mm_mesh_reg_forward", "mm_mesh_reg_backward", "mm_texture_flow_forward",
           "mm_texture_flow_backward", "mm_attribute_loss_query_workspace", "mm_attribute_loss_forward",
           "mm_attribute_loss_backward",
           "mm_prepare_vertices_query_workspace", "mm_prepare_vertices_forward", "mm_prepare_vertices_backward",
           "mm_face_normals_forward", "mm_face_normals_backward", "mm_dibr_query_workspace", "mm_dibr_rasterization_forward",
           "mm_dibr_rasterization_backward", "mm_texture_mapping_forward", "mm_texture_mapping_backward", "mm_texture_mapping_backward_query_workspace", "mm_sh_lighting_forward",
           "mm_sh_lighting_backward", "mm_mask_iou_forward", "mm_mask_iou_backward", "mm_ssim_query_workspace", "mm_ssim_forward",
           "mm_ssim_backward", "mm_shape_features_query_workspace", "mm_shape_features_forward", "mm_shape_features_backward",
           "mm_camera_features_query_workspace", "mm_camera_features_forward", "mm_camera_features_backward",
           "mm_interp_query_workspace", "mm_collapse_resample", "mm_attribute_mix_forward", "mm_attribute_mix_backward",
           "mm_render_views_query_workspace", "mm_render_views_forward", "mm_render_views_backward",
           "mm_render_indexed_query_workspace", "mm_render_indexed_forward", "mm_render_indexed_backward",
           "mm_critic_inputs_forward", "mm_critic_inputs_backward", "mm_export_images", "mm_export_grid", "mm_assemble_batch", "mm_composite_frames", "mm_pyramid_frames", "mm_jpeg_query_workspace", "mm_jpeg_files_offset", "mm_jpeg_encode", "mm_struct_size",
           "mm_abi_version")


_STRUCT_IDS = None


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
    for name in EXPORTS:
        if not hasattr(L, name):
            raise RuntimeError("libmm_render.so does not export %s" % name)
    L.mm_query_workspace.restype = ctypes.c_size_t
    L.mm_query_workspace.argtypes = [ctypes.POINTER(MMRenderDesc)]
    L.mm_render_forward.argtypes = [ctypes.POINTER(MMRenderDesc), c_p]
    L.mm_render_backward.argtypes = [ctypes.POINTER(MMRenderDesc), ctypes.POINTER(MMRenderGrads), c_p]
    L.mm_render_fused_loss.argtypes = [ctypes.POINTER(MMRenderDesc), c_p]
    L.mm_render_step_mode.argtypes = [ctypes.POINTER(MMRenderDesc)]
    L.mm_debug_step_layout.argtypes = [ctypes.POINTER(MMRenderDesc), ctypes.POINTER(ctypes.c_size_t)]
    L.mm_render_status.argtypes = [ctypes.POINTER(MMRenderDesc), c_p, ctypes.POINTER(ctypes.c_int32)]
    L.mm_recon_query_workspace.restype = ctypes.c_size_t
    L.mm_recon_query_workspace.argtypes = [ctypes.POINTER(MMReconDesc)]
    L.mm_recon_data_forward.argtypes = [ctypes.POINTER(MMReconDesc), c_p]
    L.mm_recon_data_backward.argtypes = [ctypes.POINTER(MMReconDesc), c_p]
    L.mm_recon_data_totals.restype = c_p
    L.mm_recon_data_totals.argtypes = [ctypes.POINTER(MMReconDesc)]
    L.mm_nearest_neighbour.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p]
    L.mm_chamfer_nearest.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
    L.mm_chamfer_backward.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
    L.mm_mesh_reg_query_workspace.restype = ctypes.c_size_t
    L.mm_mesh_reg_query_workspace.argtypes = [ctypes.POINTER(MMMeshRegDesc)]
    L.mm_mesh_reg_forward.argtypes = [ctypes.POINTER(MMMeshRegDesc), c_p]
    L.mm_mesh_reg_backward.argtypes = [ctypes.POINTER(MMMeshRegDesc), ctypes.POINTER(MMMeshRegGrads), c_p]
    L.mm_attribute_loss_query_workspace.restype = ctypes.c_size_t
    L.mm_attribute_loss_query_workspace.argtypes = [ctypes.POINTER(MMAttLossDesc)]
    L.mm_attribute_loss_forward.argtypes = [ctypes.POINTER(MMAttLossDesc), c_p]
    L.mm_attribute_loss_backward.argtypes = [ctypes.POINTER(MMAttLossDesc), ctypes.POINTER(MMAttLossGrads), c_p]
    L.mm_texture_flow_forward.argtypes = [ctypes.POINTER(MMTexFlowDesc), c_p]
    L.mm_texture_flow_backward.argtypes = [ctypes.POINTER(MMTexFlowDesc), ctypes.POINTER(MMTexFlowGrads), c_p]
    P = ctypes.POINTER
    L.mm_prepare_vertices_query_workspace.restype = ctypes.c_size_t
    L.mm_prepare_vertices_query_workspace.argtypes = [P(MMPrepareDesc)]
    L.mm_prepare_vertices_forward.argtypes = [P(MMPrepareDesc), c_p]
    L.mm_prepare_vertices_backward.argtypes = [P(MMPrepareDesc), P(MMPrepareGrads), c_p]
    L.mm_face_normals_forward.argtypes = [ctypes.c_int64, c_i, c_p, c_p, c_p]
    L.mm_face_normals_backward.argtypes = [ctypes.c_int64, c_i, c_p, c_p, c_p, c_p]
    L.mm_dibr_query_workspace.restype = ctypes.c_size_t
    L.mm_dibr_query_workspace.argtypes = [P(MMDibrDesc)]
    L.mm_dibr_rasterization_forward.argtypes = [P(MMDibrDesc), c_p]
    L.mm_dibr_rasterization_backward.argtypes = [P(MMDibrDesc), P(MMDibrGrads), c_p]
    L.mm_texture_mapping_forward.argtypes = [P(MMTexMapDesc), c_p]
    L.mm_texture_mapping_backward.argtypes = [P(MMTexMapDesc), P(MMTexMapGrads), c_p]
    L.mm_texture_mapping_backward_query_workspace.argtypes = [P(MMTexMapDesc)]
    L.mm_texture_mapping_backward_query_workspace.restype = ctypes.c_size_t
    L.mm_sh_lighting_forward.argtypes = [P(MMShDesc), c_p]
    L.mm_sh_lighting_backward.argtypes = [P(MMShDesc), P(MMShGrads), c_p]
    L.mm_mask_iou_forward.argtypes = [P(MMMaskIouDesc), c_p]
    L.mm_mask_iou_backward.argtypes = [P(MMMaskIouDesc), c_p, c_p, c_p, c_p]
    L.mm_ssim_query_workspace.restype = ctypes.c_size_t
    L.mm_ssim_query_workspace.argtypes = [P(MMSsimDesc)]
    L.mm_ssim_forward.argtypes = [P(MMSsimDesc), c_p]
    L.mm_ssim_backward.argtypes = [P(MMSsimDesc), P(MMSsimGrads), c_p]
    L.mm_shape_features_query_workspace.restype = ctypes.c_size_t
    L.mm_shape_features_query_workspace.argtypes = [P(MMShapeFeatDesc)]
    L.mm_shape_features_forward.argtypes = [P(MMShapeFeatDesc), c_p]
    L.mm_shape_features_backward.argtypes = [P(MMShapeFeatDesc), P(MMShapeFeatGrads), c_p]
    L.mm_camera_features_query_workspace.restype = ctypes.c_size_t
    L.mm_camera_features_query_workspace.argtypes = [P(MMCameraFeatDesc)]
    L.mm_camera_features_forward.argtypes = [P(MMCameraFeatDesc), c_p]
    L.mm_camera_features_backward.argtypes = [P(MMCameraFeatDesc), P(MMCameraFeatGrads), c_p]
    L.mm_interp_query_workspace.restype = ctypes.c_size_t
    L.mm_interp_query_workspace.argtypes = [P(MMInterpDesc)]
    L.mm_collapse_resample.argtypes = [c_i, c_i, c_p, c_p, c_p, c_p, c_f, c_p, c_p]
    L.mm_attribute_mix_forward.argtypes = [P(MMInterpDesc), c_p]
    L.mm_attribute_mix_backward.argtypes = [P(MMInterpDesc), P(MMInterpGrads), c_p]
    L.mm_render_views_query_workspace.restype = ctypes.c_size_t
    L.mm_render_views_query_workspace.argtypes = [P(MMRenderViewsDesc)]
    L.mm_render_views_forward.argtypes = [P(MMRenderViewsDesc), c_p]
    L.mm_render_views_backward.argtypes = [P(MMRenderViewsDesc), P(MMRenderGrads), c_p]
    L.mm_render_indexed_query_workspace.restype = ctypes.c_size_t
    L.mm_render_indexed_query_workspace.argtypes = [P(MMRenderIndexedDesc)]
    L.mm_render_indexed_forward.argtypes = [P(MMRenderIndexedDesc), c_p]
    L.mm_render_indexed_backward.argtypes = [P(MMRenderIndexedDesc), P(MMRenderGrads), c_p]
    L.mm_critic_inputs_forward.argtypes = [P(MMCriticDesc), c_p]
    L.mm_critic_inputs_backward.argtypes = [P(MMCriticDesc), P(MMCriticGrads), c_p]
    L.mm_export_images.argtypes = [P(MMExportDesc), c_p]
    L.mm_export_grid.argtypes = [P(MMExportDesc), c_p]
    L.mm_assemble_batch.argtypes = [P(MMBatchDesc), c_p]
    L.mm_composite_frames.argtypes = [P(MMCompositeDesc), c_p]
    L.mm_pyramid_frames.argtypes = [P(MMPyramidDesc), c_p]
    L.mm_jpeg_query_workspace.restype = ctypes.c_size_t
    L.mm_jpeg_query_workspace.argtypes = [P(MMJpegDesc)]
    L.mm_jpeg_files_offset.restype = ctypes.c_size_t
    L.mm_jpeg_files_offset.argtypes = [P(MMJpegDesc)]
    L.mm_jpeg_encode.argtypes = [P(MMJpegDesc), c_p]
    L.mm_struct_size.restype = ctypes.c_size_t
    L.mm_struct_size.argtypes = [ctypes.c_int]
    L.mm_build_vertex_corner_csr.argtypes = [c_i, c_i, c_p, c_p, c_p]
    L.mm_build_vertex_corner_csr_device.argtypes = [c_i, c_i, c_p, c_p, c_p, c_p, c_p]
    L.mm_status_string.restype = ctypes.c_char_p
    L.mm_status_string.argtypes = [ctypes.c_int]
    L.mm_last_error_detail.restype = ctypes.c_char_p
    L.mm_last_error_detail.argtypes = []
    L.mm_abi_version.restype = ctypes.c_int
    if L.mm_abi_version() != ABI_VERSION:
        raise RuntimeError("libmm_render.so has ABI version %d, this binding mirrors version %d" % (L.mm_abi_version(), ABI_VERSION))
    mirrors = (MMRenderDesc, MMRenderGrads, MMReconDesc, MMMeshRegDesc, MMMeshRegGrads, MMAttLossDesc, MMAttLossGrads, MMTexFlowDesc,
               MMTexFlowGrads, MMPrepareDesc, MMPrepareGrads, MMDibrDesc, MMDibrGrads, MMTexMapDesc, MMTexMapGrads, MMShDesc, MMShGrads,
               MMMaskIouDesc, MMSsimDesc, MMSsimGrads, MMShapeFeatDesc, MMShapeFeatGrads, MMCameraFeatDesc, MMCameraFeatGrads,
               MMInterpDesc, MMInterpGrads, MMRenderViewsDesc, MMCriticDesc, MMCriticGrads, MMExportDesc, MMBatchDesc,
               None, MMCompositeDesc, MMRenderIndexedDesc, None, MMPyramidDesc, None, MMJpegDesc)        # (ids 31, 34 and 36 are unassigned)
    for i, cls in enumerate(mirrors):
        if cls is not None and L.mm_struct_size(i) != ctypes.sizeof(cls):
            raise RuntimeError("struct layout mismatch for %s: library %d bytes, binding %d" % (cls.__name__, L.mm_struct_size(i), ctypes.sizeof(cls)))
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


def upload_int32(values, device):
    """int32 ``values`` (a tensor, or an array that is cast) to ``device`` through pinned host memory, without waiting: (host, dev).  A
    descriptor may name the pinned copy as its host table; it is read before the call returns."""
    src = values if torch.is_tensor(values) else torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32))
    host = torch.empty(src.shape, dtype=torch.int32, pin_memory=True)
    host.copy_(src)
    return host, host.to(device, non_blocking=True)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream(device):
    """The current HIP stream of ``device`` as a void* (the raw-handle query when torch offers it: the Stream object costs microseconds)."""
    if _raw_stream is not None and device.index is not None:
        return ctypes.c_void_p(_raw_stream(device.index))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("the MI355X render path needs tensors in device memory (got a %s tensor); "
                               "there is no CPU fallback" % t.device)
