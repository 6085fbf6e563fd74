"""SURVEY.md 8(b) row 2, the import boundary: with 3d-magic-mirror_amd/shim on sys.path every kaolin / pytorch3d name the reference
imports at module top (networks.py:6-19, trainer.py:31-40) resolves against this repo's package, with the signatures its call sites use.
The names and signatures are restated here; the shim provides kaolin and pytorch3d, nothing else."""
import inspect
import os
import sys

from conftest import ROOT

SHIM = os.path.join(ROOT, "3d-magic-mirror_amd", "shim")


def test_shim_exposes_the_names_and_signatures_the_reference_uses():
    sys.path.insert(0, SHIM)
    try:
        import kaolin as kal
        from kaolin.render.camera import generate_perspective_projection
        from kaolin.render.mesh import dibr_rasterization, prepare_vertices, spherical_harmonic_lighting, texture_mapping
        from kaolin.metrics.render import mask_iou
        from pytorch3d.loss import chamfer_distance
    finally:
        sys.path.remove(SHIM)
    assert kal.io.obj.import_mesh and kal.ops.mesh.index_vertices_by_faces and kal.ops.mesh.uniform_laplacian and kal.ops.mesh.face_normals
    assert kal.metrics.render.mask_iou is mask_iou
    p = inspect.signature(dibr_rasterization).parameters
    assert list(p)[:6] == ["height", "width", "face_vertices_z", "face_vertices_image", "face_features", "face_normals_z"]
    assert (p["sigmainv"].default, p["boxlen"].default, p["knum"].default, p["multiplier"].default, p["eps"].default,
            p["rast_backend"].default) == (7000, 0.02, 30, None, None, "cuda")
    assert list(inspect.signature(prepare_vertices).parameters) == ["vertices", "faces", "camera_proj", "camera_rot", "camera_trans", "camera_transform"]
    assert inspect.signature(texture_mapping).parameters["mode"].default == "nearest"
    assert list(inspect.signature(spherical_harmonic_lighting).parameters) == ["imnormal", "lights"]
    assert list(inspect.signature(mask_iou).parameters) == ["lhs_mask", "rhs_mask"]
    assert list(inspect.signature(generate_perspective_projection).parameters)[:2] == ["fovyangle", "ratio"]
    assert list(inspect.signature(chamfer_distance).parameters)[:2] == ["x", "y"]
    assert list(inspect.signature(kal.ops.mesh.face_normals).parameters) == ["face_vertices", "unit"]
    assert list(inspect.signature(kal.io.obj.import_mesh).parameters)[:2] == ["path", "with_materials"]
    for m in ("kaolin", "pytorch3d"):                            # leave the interpreter as found for the other tests
        for k in [k for k in sys.modules if k == m or k.startswith(m + ".")]:
            del sys.modules[k]
