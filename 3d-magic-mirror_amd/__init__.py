"""MI355X-native differentiable render + reconstruction-loss path for 3D-Magic-Mirror (gfx950 HIP kernels behind a
C ABI; the host side mirrors the reference's DiffRender API).  Import as ``importlib.import_module('3d-magic-mirror_amd')``
or through the root-level ``mm_amd`` alias."""
from . import encoder_features, interpolate, mesh_reg, obj_io, template, texture_flow, synthetic  # noqa: F401
from .diff_render import DiffRender, check_render_index, deep_copy, grid_index  # noqa: F401
from .obj_io import import_mesh, save_mesh  # noqa: F401
from .texture_flow import sample_texture  # noqa: F401
from .encoder_features import camera_features, shape_features  # noqa: F401
from .critic_inputs import CriticInputs, critic_inputs  # noqa: F401
from .disentangle import disentangle_inputs, disentangle_terms, draw_erase_box  # noqa: F401
from .export import export_grid, export_images, grid_shape  # noqa: F401
from .composite import composite_frames, gaussian_taps, lower_composite, resize_taps  # noqa: F401
from .pyramid import lower_pyramid, pyramid_frames  # noqa: F401
from .poisson import lower_poisson, poisson_frames  # noqa: F401
from .jpeg import JpegBatch, encode_jpeg, jpeg_roundtrip, lower_jpeg  # noqa: F401
from .jpeg_decode import DecodedFrames, decode_jpeg, decode_jpeg_host, lower_jpeg_decode  # noqa: F401
from .png_decode import decode_png, decode_png_host, lower_png_decode  # noqa: F401
from .gif import GIF_SEGMENT, GifFile, encode_gif, quantize_frames  # noqa: F401
from .png import PNG_MAX_SEGMENT, PNG_SEGMENT, PngBatch, encode_png, lower_png  # noqa: F401
from .fid import FID_SPLIT, FidStatistics, fid_score, frechet_distance, inception_input  # noqa: F401
from .input_batches import ImagePool, assemble_batch, assemble_records, draw_augmentation, lower_batch  # noqa: F401
from .interpolate import interpolate_attributes, mix_attributes, resample_collapsed  # noqa: F401
from .ssim import MS_SSIM, SSIM, ms_ssim, recon_scores, recon_scores_as_saved, ssim  # noqa: F401
