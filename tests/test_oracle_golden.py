"""Pins the CPU oracle and the host-side template logic against fixtures minted from the importable parts of the
reference (tests/golden/make_golden.py): smr_utils camera math, DiffRender.__init__, DiffRender.recon_data."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, TEMPLATES, load_template_npz


def test_camera_matches_smr_utils(oracle):
    z = np.load(os.path.join(GOLDEN, "camera.npz"))
    T = oracle.camera(z["dist"], z["elev"], z["azim"], z["bias"])
    np.testing.assert_allclose(T, z["transform"], rtol=0, atol=2e-6)
    # camera position is recoverable: t = -cam @ R  =>  cam = -t @ R^T
    cam = -np.einsum("bj,bij->bi", T[:, 3], T[:, :3])
    np.testing.assert_allclose(cam, z["camera_position"], atol=5e-6)
    T64 = oracle.camera(z["dist"], z["elev"], z["azim"], z["bias"], dtype=np.float64)
    np.testing.assert_allclose(T64, z["transform"], atol=2e-6)


@pytest.mark.parametrize("name,ell,ratio", [("sphere", 1, 1), ("smpl_uv_642", 1, 1), ("ellipsoid", 1, 1),
                                            ("smpl_uv_642", 2, 2), ("sphere", -1, 1)])
def test_template_prep_matches_reference_init(pkg, name, ell, ratio):
    t = pkg.template
    z = np.load(os.path.join(GOLDEN, "template_%s_e%d_r%d.npz" % (name, ell, ratio)))
    m = load_template_npz(name)
    v = t.normalize_template(torch.from_numpy(m["vertices"]), ell)
    np.testing.assert_array_equal(v.numpy(), z["vertices_init"])
    np.testing.assert_array_equal(t.flip_pairing(v).numpy(), z["flip_index"])
    faces = torch.from_numpy(m["faces"]).long()
    edges, e2f = t.edge_tables(faces)
    np.testing.assert_array_equal(edges.numpy(), z["edges"])
    np.testing.assert_array_equal(np.sort(e2f.numpy(), axis=1), z["edge2faces_sorted"])
    fu = t.index_vertices_by_faces(torch.from_numpy(m["uvs"])[None], torch.from_numpy(m["face_uvs_idx"]).long())
    np.testing.assert_array_equal(fu.numpy(), z["face_uvs"])
    proj = t.generate_perspective_projection(np.arctan(1.0 / 2.5) * 2, ratio=1 / ratio)
    np.testing.assert_array_equal(proj.numpy(), z["cam_proj"])
    L = t.uniform_laplacian(v.shape[0], faces)
    np.testing.assert_allclose(L.sum(1).numpy(), z["laplacian_rowsum"], atol=1e-6)
    assert int((L != 0).sum()) == int(z["laplacian_nnz"])
    np.testing.assert_array_equal(torch.sign(v[:, 2]).numpy(), z["sign_init"])
    # CSR forms agree with the dense/reference tables
    off, items = t.vertex_corner_adjacency(v.shape[0], faces)
    flat = faces.reshape(-1).numpy()
    for vid in (0, 17, v.shape[0] - 1):
        assert set(items[off[vid]:off[vid + 1]].tolist()) == set(np.flatnonzero(flat == vid).tolist())
    loff, lnb = t.sparse_laplacian_rows(v.shape[0], faces)
    for vid in (0, 5, v.shape[0] - 1):
        assert set(lnb[loff[vid]:loff[vid + 1]].tolist()) == set(np.flatnonzero(L[vid].numpy() > 0).tolist())


# OBJ text of a template fixture, laid out like the reference's own template files: "a/b" corners (sphere, ellipsoid; the ellipsoid's
# "v" records end in a blank), a header with mtllib / usemtl, "vn" records and "a/b/c" corners (smpl_uv_642), "a/b/c" corners naming no
# "vn" record and a doubled separator (smpl_uv)
OBJ_STYLES = {"sphere": {}, "ellipsoid": {"v_tail": " "}, "smpl_uv_642": {"header": True, "vn": True, "corner": "abc"},
              "smpl_uv": {"header": True, "corner": "abc", "sep": ["  ", " "]}}


def write_template_obj(name, path):
    """Writes tests/golden/templates/<name>.npz as an OBJ file (shortest float32 decimals, 1-based indices); returns the path."""
    m = load_template_npz(name)
    st = OBJ_STYLES[name]
    num = lambda x: np.format_float_positional(np.float32(x), unique=True, trim="0")
    out = ["# template mesh %s\n" % name, "mtllib %s.obj.mtl\n" % name, "usemtl material_0\n", "\n"] if st.get("header") else []
    out += ["v %s %s %s%s\n" % (num(a), num(b), num(c), st.get("v_tail", "")) for a, b, c in m["vertices"]]
    if st.get("vn"):
        out += ["vn 0 0 1\n"] * len(m["vertices"])
    out += ["vt %s %s\n" % (num(a), num(b)) for a, b in m["uvs"]]
    sep = st.get("sep", [" ", " "])
    for f, t in zip(m["faces"] + 1, m["face_uvs_idx"] + 1):
        c = ["%d/%d/%d" % (f[k], t[k], f[k]) if st.get("corner") == "abc" else "%d/%d" % (f[k], t[k]) for k in range(3)]
        out.append("f " + c[0] + sep[1] + c[1] + sep[0] + c[2] + "\n")
    path.write_text("".join(out))
    return str(path)


@pytest.mark.parametrize("name", ["sphere", "smpl_uv_642", "ellipsoid"])
def test_obj_parser_reproduces_template_fixture(pkg, name, tmp_path):
    m = pkg.obj_io.import_mesh(write_template_obj(name, tmp_path / (name + ".obj")))
    z = load_template_npz(name)
    np.testing.assert_array_equal(m.vertices.numpy(), z["vertices"])
    np.testing.assert_array_equal(m.faces.numpy(), z["faces"])
    np.testing.assert_array_equal(m.uvs.numpy(), z["uvs"])
    np.testing.assert_array_equal(m.face_uvs_idx.numpy(), z["face_uvs_idx"])


def test_obj_roundtrip_and_edge_cases(pkg, tmp_path):
    p = tmp_path / "t.obj"
    p.write_text("# c\nmtllib x.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nvt 0 0\nvt 1 0\nvt 0 1\nvn 0 0 1\n"
                 "f 1/1/1 2/2/1 3/3/1\nf -1/1 -2/2 -3/3\nf 1 2 4\n")
    m = pkg.obj_io.import_mesh(str(p))
    assert m.vertices.shape == (4, 3) and m.faces.tolist() == [[0, 1, 2], [3, 2, 1], [0, 1, 3]]
    assert m.face_uvs_idx.tolist() == [[0, 1, 2], [0, 1, 2], [-1, -1, -1]]
    q = tmp_path / "o.obj"
    pkg.obj_io.save_mesh(str(q), m.vertices, m.faces, m.uvs)
    m2 = pkg.obj_io.import_mesh(str(q))
    np.testing.assert_allclose(m2.vertices.numpy(), m.vertices.numpy())
    assert m2.faces.tolist() == m.faces.tolist() and m2.uvs.shape == (3, 2)
    (tmp_path / "quad.obj").write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3 4\n")
    with pytest.raises(ValueError):
        pkg.obj_io.import_mesh(str(tmp_path / "quad.obj"))
    npz = pkg.obj_io.load_template(os.path.join(TEMPLATES, "sphere.npz"))
    assert npz.vertices.shape == (642, 3) and npz.faces.dtype == torch.int64


@pytest.mark.parametrize("contour", [0.0, 0.5])
def test_recon_data_matches_reference(oracle, contour):
    z = np.load(os.path.join(GOLDEN, "losses.npz"))
    pred = z["rd_pred_nhwc"].transpose(0, 3, 1, 2)          # NCHW view of NHWC storage, like render's output
    for dt, tol in ((np.float32, 2e-6), (np.float64, 1e-6)):
        loss, dpred = oracle.recon_data(pred.astype(dt).transpose(0, 2, 3, 1).copy().transpose(0, 3, 1, 2), z["rd_gt"],
                                        image_weight=0.1, contour=contour, want_grad=True, dtype=dt)
        assert abs(loss - float(z["recon_data_c%g" % contour])) < tol
        np.testing.assert_allclose(dpred.transpose(0, 2, 3, 1), z["recon_data_c%g__d_pred_nhwc" % contour], rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("name", ["sphere", "smpl_uv_642", "ellipsoid", "smpl_uv"])
def test_template_helpers_against_independent_restatements(pkg, name, tmp_path):
    """The three kaolin helpers DiffRender.__init__ calls (import_mesh, uniform_laplacian, generate_perspective_projection; networks.py:172-249)
    are this repo's own code in the template fixtures too (tools/make_golden.py mints through them: kaolin is not in the image).  Here each is
    checked against a second, differently built restatement that shares no code with the first: a regular-expression OBJ reader, a
    scipy.sparse adjacency, the pinhole formula written out.  The OBJ text is written from the template's fixture (write_template_obj)."""
    import re
    import scipy.sparse as sp
    path = write_template_obj(name, tmp_path / (name + ".obj"))
    # -- OBJ: v / vt / f a/b[/c] records, 1-based indices
    vs, vts, fs, fts = [], [], [], []
    for line in open(path):
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "v":
            vs.append([float(x) for x in tok[1:4]])
        elif tok[0] == "vt":
            vts.append([float(x) for x in tok[1:3]])
        elif tok[0] == "f":
            refs = [re.match(r"(-?\d+)(?:/(-?\d*))?", t).groups() for t in tok[1:]]
            assert len(refs) == 3
            fs.append([int(r[0]) - 1 for r in refs])
            fts.append([int(r[1]) - 1 if r[1] else -1 for r in refs])
    m = pkg.obj_io.import_mesh(path)
    np.testing.assert_array_equal(m.vertices.numpy(), np.asarray(vs, np.float32))
    np.testing.assert_array_equal(m.faces.numpy(), np.asarray(fs, np.int64))
    np.testing.assert_array_equal(m.uvs.numpy(), np.asarray(vts, np.float32))
    np.testing.assert_array_equal(m.face_uvs_idx.numpy(), np.asarray(fts, np.int64))
    # -- uniform Laplacian: row-normalised vertex adjacency minus the identity
    f = np.asarray(fs, np.int64)
    V = len(vs)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    A = sp.coo_matrix((np.ones(2 * len(e)), (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=(V, V)).tocsr()
    A.data[:] = 1.0                                               # an edge shared by two faces is one neighbour
    deg = np.asarray(A.sum(1)).reshape(-1)
    Lref = (sp.diags(1.0 / np.maximum(deg, 1)) @ A - sp.identity(V)).toarray().astype(np.float32)
    np.testing.assert_allclose(pkg.template.uniform_laplacian(V, torch.from_numpy(f)).numpy(), Lref, rtol=0, atol=1e-7)
    # -- perspective projection of a pinhole with vertical field of view fovy and width/height = ratio: x' = x / (ratio tan), y' = y / tan, z' = -z
    for fovy, ratio in ((np.arctan(1.0 / 2.5) * 2, 1.0), (0.9, 0.5), (1.3, 2.0)):
        p = pkg.template.generate_perspective_projection(fovy, ratio=ratio).numpy().reshape(3)
        np.testing.assert_allclose(p, [np.cos(fovy / 2) / (ratio * np.sin(fovy / 2)), np.cos(fovy / 2) / np.sin(fovy / 2), -1.0], rtol=1e-6)
