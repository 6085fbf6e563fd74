"""CPU-side checks of the product: the C-ABI library loads and exports every symbol include/mm_render.h declares, the
host helpers of the ABI work, and the torch-restated losses of the DiffRender mirror match the reference's own outputs
(tests/golden/losses.npz, minted by running /root/reference/networks.py under kaolin stubs)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, TEMPLATES

N_MAX_D = 32          # MM_DIBR_MAX_D


def test_library_exports_every_declared_symbol(pkg):
    hdr = open(os.path.join(ROOT, "include", "mm_render.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char\*|const float\*)\s+(mm_\w+)\s*\(", hdr, flags=re.M))
    assert {"mm_render_forward", "mm_render_backward", "mm_recon_data_forward", "mm_recon_data_backward",
            "mm_query_workspace", "mm_recon_query_workspace", "mm_build_vertex_corner_csr", "mm_dibr_rasterization_forward",
            "mm_prepare_vertices_forward", "mm_texture_mapping_forward", "mm_sh_lighting_forward", "mm_mask_iou_forward"} <= declared
    from importlib import import_module
    N = import_module("3d-magic-mirror_amd._native")
    lib = N.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert set(N.EXPORTS) == declared
    assert lib.mm_abi_version() == N.ABI_VERSION == int(re.search(r"#define MM_ABI_VERSION (\d+)", hdr).group(1))
    # every struct the header declares is mirrored field for field: same size as the library compiled it (N.lib() also checks)
    names = re.findall(r"^typedef struct (MM\w+) \{", hdr, flags=re.M)
    ids = re.search(r"Ids: (.*?)\. \*/", hdr, flags=re.S).group(1).replace("\n", " ").replace("*", " ")
    table = {m.group(2): int(m.group(1)) for m in re.finditer(r"(\d+) (MM\w+)", ids)}
    assert set(names) - {"MMAttributes"} == set(table), (sorted(names), sorted(table))
    for nm, i in table.items():
        assert lib.mm_struct_size(i) == ctypes.sizeof(getattr(N, nm)) > 0, nm
    assert lib.mm_struct_size(99) == 0
    assert lib.mm_status_string(-3).decode().startswith("workspace")
    assert lib.mm_last_error_detail().decode() == ""            # nothing launched, nothing recorded
    # struct layout agrees with the header (the library sizes the workspace from the same struct)
    d = N.MMRenderDesc()
    d.B, d.H, d.W, d.V, d.F, d.Ht, d.Wt = 2, 64, 64, 642, 1280, 128, 64
    ws = lib.mm_query_workspace(ctypes.byref(d))
    assert ws > 0 and ws % 256 == 0
    d.B = 0
    assert lib.mm_query_workspace(ctypes.byref(d)) == 0
    # argument validation happens before any GPU work
    assert lib.mm_render_forward(ctypes.byref(d), None) == -2            # MM_ERR_BAD_SHAPE
    assert lib.mm_render_forward(None, None) == -1                       # MM_ERR_NULL_POINTER
    r = N.MMReconDesc()
    assert lib.mm_recon_data_forward(ctypes.byref(r), None) == -2
    # the op boundary validates before launching too
    assert lib.mm_dibr_rasterization_forward(None, None) == -1 and lib.mm_dibr_rasterization_forward(ctypes.byref(N.MMDibrDesc()), None) == -2
    q = N.MMDibrDesc(); q.B, q.H, q.W, q.F, q.D, q.knum = 1, 8, 8, 4, N_MAX_D + 1, 30
    assert lib.mm_dibr_rasterization_forward(ctypes.byref(q), None) == -5                # MM_ERR_UNSUPPORTED: too many channels
    q.D = 3
    assert lib.mm_dibr_query_workspace(ctypes.byref(q)) % 256 == 0 and lib.mm_dibr_rasterization_forward(ctypes.byref(q), None) == -1
    assert lib.mm_prepare_vertices_forward(ctypes.byref(N.MMPrepareDesc()), None) == -2
    assert lib.mm_texture_mapping_forward(ctypes.byref(N.MMTexMapDesc()), None) == -2
    assert lib.mm_sh_lighting_forward(ctypes.byref(N.MMShDesc()), None) == -2
    assert lib.mm_mask_iou_forward(ctypes.byref(N.MMMaskIouDesc()), None) == -2
    assert lib.mm_face_normals_forward(0, 1, None, None, None) == -1


def test_signature_table_is_the_headers(pkg):
    """N.SIGNATURES, the binding's one declaration of the C ABI, against every function include/mm_render.h declares: the same names, as many
    argtypes as parameters, the restype of the return type, POINTER(mirror) wherever a descriptor goes in -- and the loaded library carries it."""
    N = pkg._native
    hdr = open(os.path.join(ROOT, "include", "mm_render.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decls = re.findall(r"^(int|size_t|const char\*|const float\*)\s+(mm_\w+)\s*\((.*?)\)\s*;", code, flags=re.M | re.S)
    assert len(decls) == len({name for _, name, _ in decls}) >= 74
    restypes = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p, "const float*": ctypes.c_void_p}
    lib = N.lib()
    for ret, name, params in decls:
        assert name in N.SIGNATURES, name
        restype, argtypes = N.SIGNATURES[name]
        params = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        assert len(argtypes) == len(params), (name, params)
        assert restype is restypes[ret], name
        for k, p in enumerate(params):
            m = re.fullmatch(r"const (MM\w+)\* \w+", p)
            if m:
                assert argtypes[k] is ctypes.POINTER(getattr(N, m.group(1))), (name, p)
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    assert set(N.SIGNATURES) == {name for _, name, _ in decls}
    assert N.EXPORTS == tuple(N.SIGNATURES)


def test_struct_ids_are_the_headers(pkg):
    """N.STRUCT_IDS, what lib() holds against mm_struct_size, is the header's "Ids:" list; the unassigned ids are absent, not padded."""
    N = pkg._native
    hdr = open(os.path.join(ROOT, "include", "mm_render.h")).read()
    ids = re.search(r"Ids: (.*?)\. \*/", hdr, flags=re.S).group(1).replace("\n", " ").replace("*", " ")
    table = {int(m.group(1)): getattr(N, m.group(2)) for m in re.finditer(r"(\d+) (MM\w+)", ids)}
    assert len(table) >= 35 and N.STRUCT_IDS == table
    assert not {31, 34, 36} & set(N.STRUCT_IDS)
    assert not hasattr(N, "_STRUCT_IDS")


def test_call_path_raises_with_the_entry_points_name(pkg):
    """N.call: the status of a refusal becomes check's RuntimeError under the export's name (or ``what``), an unknown name raises before anything
    is called, and a Python int where a pointer belongs is an ArgumentError instead of a truncated address -- for every export, the two
    debug/host helpers that once had no argtypes included.  The all-zero descriptor is refused by the shape check before any launch."""
    N = pkg._native
    null = ctypes.c_void_p(0)
    with pytest.raises(RuntimeError) as e:
        N.call("mm_ssim_forward", null, N.MMSsimDesc())
    assert str(e.value) == "mm_ssim_forward failed: bad or inconsistent size (MMStatus -2)"
    with pytest.raises(RuntimeError) as e:
        N.call("mm_ssim_forward", null, N.MMSsimDesc(), what="label")
    assert str(e.value) == "label failed: bad or inconsistent size (MMStatus -2)"
    with pytest.raises(RuntimeError, match="mm_no_such_entry is not an export"):
        N.call("mm_no_such_entry", null, N.MMSsimDesc())
    addr = ctypes.addressof(N.MMSsimDesc())
    with pytest.raises(ctypes.ArgumentError):
        N.call("mm_ssim_forward", null, addr)
    out = (ctypes.c_size_t * 16)()
    with pytest.raises(ctypes.ArgumentError):
        N.fn("mm_debug_workspace_layout")(addr, out)
    with pytest.raises(ctypes.ArgumentError):
        N.fn("mm_debug_workspace_layout")(N.MMRenderDesc(), ctypes.addressof(out))
    with pytest.raises(ctypes.ArgumentError):
        N.fn("mm_build_vertex_corner_table")(4, 2, None, 0.5, None)                  # (its stride is an int32, not whatever came)
    assert N.fn("mm_debug_workspace_layout")(None, out) == -1                        # typed, it still answers: MM_ERR_NULL_POINTER
    assert N.fn("mm_last_error_detail")().decode() == ""                              # nothing was launched


def test_option_bits_of_the_binding_are_the_headers(pkg):
    """Every MM_OPT_* bit include/mm_render.h declares has its OPT_* twin in the ctypes binding with the same value, and no two share a bit."""
    hdr = open(os.path.join(ROOT, "include", "mm_render.h")).read()
    bits = {m.group(1): 1 << int(m.group(2)) for m in re.finditer(r"MM_OPT_([A-Z_]+)\s*=\s*1\s*<<\s*(\d+)", hdr)}
    assert len(bits) >= 11 and "MANY_IN_FLIGHT" in bits
    assert len(set(bits.values())) == len(bits)
    for name, value in bits.items():
        assert getattr(pkg._native, "OPT_" + name) == value, name


def test_host_csr_builders(pkg):
    from importlib import import_module
    N = import_module("3d-magic-mirror_amd._native")
    lib = N.lib()
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), 32)
    faces = dr.faces.numpy().astype(np.int32)
    V, F = dr.num_vertices, dr.num_faces
    off = np.zeros(V + 1, np.int32); items = np.zeros(3 * F, np.int32)
    assert lib.mm_build_vertex_corner_csr(V, F, faces.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p),
                                          items.ctypes.data_as(ctypes.c_void_p)) == 0
    ro, ri = pkg.template.vertex_corner_adjacency(V, dr.faces)
    np.testing.assert_array_equal(off, ro.numpy()); np.testing.assert_array_equal(items, ri.numpy())
    # the fixed-stride form MMRenderDesc.vc_table takes: the library's helper and the host class build the same table, which lists, per
    # vertex, exactly the CSR's corners (ascending) together with their faces' vertex ids
    for name in ("sphere", "smpl_uv_642", "smpl_uv"):
        d2 = pkg.DiffRender(os.path.join(TEMPLATES, name + ".npz"), 32)
        f2 = d2.faces.numpy().astype(np.int32)
        V2, F2 = d2.num_vertices, d2.num_faces
        stride = lib.mm_build_vertex_corner_table(V2, F2, f2.ctypes.data_as(ctypes.c_void_p), 0, None)
        tab = np.zeros((V2, stride, 4), np.int32)
        assert stride == int(np.bincount(f2.reshape(-1), minlength=V2).max())
        assert lib.mm_build_vertex_corner_table(V2, F2, f2.ctypes.data_as(ctypes.c_void_p), stride, tab.ctypes.data_as(ctypes.c_void_p)) == 0
        np.testing.assert_array_equal(tab, d2._vc_table.numpy())
        o2, i2 = pkg.template.vertex_corner_adjacency(V2, d2.faces)
        o2, i2 = o2.numpy(), i2.numpy()
        for v in (0, 1, V2 // 2, V2 - 1):
            n = o2[v + 1] - o2[v]
            np.testing.assert_array_equal(tab[v, :n, 0], i2[o2[v]:o2[v + 1]])
            assert (tab[v, n:] == -1).all() and (f2[tab[v, :n, 0] // 3] == tab[v, :n, 1:]).all()
            assert (f2.reshape(-1)[tab[v, :n, 0]] == v).all()
        assert lib.mm_build_vertex_corner_table(V2, F2, f2.ctypes.data_as(ctypes.c_void_p), stride - 1, tab.ctypes.data_as(ctypes.c_void_p)) == -2


def test_the_autograd_nodes_extension_loads_and_mirrors_the_descriptor(pkg):
    """lib/mm_torch_ext.so, the class API's only host path, loads without a GPU and was built against this binding's MMRenderDesc."""
    N = pkg._native
    ext = N.torch_ext()
    assert ext is not None and ext.desc_bytes() == ctypes.sizeof(N.MMRenderDesc)
    for name in ("render", "recon_data", "render_geometry", "deferrable"):
        assert callable(getattr(ext, name)), name


def test_render_without_gpu_fails_loudly(pkg):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), 32)
    att, gt = pkg.synthetic.synthetic_batch(dr.vertices_init, 2, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dr.render(no_mask=True, **att)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dr.recon_data(gt, gt)


def _att(z, prefix, grad=True):
    a = {k: torch.from_numpy(z[prefix + "_" + k]).clone().requires_grad_(grad)
         for k in ("delta_vertices", "face_normals", "azimuths", "elevations", "distances", "biases", "textures", "lights")}
    return a


def test_loss_oracle_and_attribute_losses_match_reference(pkg):
    """oracle/reg_oracle.py (the checker of the HIP mesh-regulariser and attribute-loss kernels) against outputs and gradients of
    the reference itself (tests/golden/losses.npz)."""
    import reg_oracle as R
    z = np.load(os.path.join(GOLDEN, "losses.npz"))
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), 64, image_weight=0.1, lambda_lpl=0.1, lambda_flat=0.001)
    dr.sign_init = dr.sign_init.cpu()
    A, A2 = _att(z, "A"), _att(z, "A2", grad=False)
    A["vertices"] = dr.vertices_init[None] + A["delta_vertices"]
    A2["vertices"] = dr.vertices_init[None] + A2["delta_vertices"]

    def check(name, value, wrt):
        np.testing.assert_allclose(value.detach().numpy(), z[name], rtol=2e-5, atol=1e-7)
        grads = torch.autograd.grad(value, [A[k] for k in wrt], allow_unused=True, retain_graph=True)
        for k, g in zip(wrt, grads):
            ref = z[name + "__d_" + k]
            got = np.zeros_like(ref) if g is None else g.numpy()
            np.testing.assert_allclose(got, ref, rtol=2e-4, atol=1e-7, err_msg=name + " d/d" + k)

    check("calc_reg_loss", R.calc_reg_loss(dr, A), ("delta_vertices", "face_normals"))
    check("calc_reg_edge", R.calc_reg_edge(dr, A["vertices"]), ("delta_vertices",))
    check("calc_reg_depth", R.calc_reg_depth(dr, A["vertices"]), ("delta_vertices",))
    check("calc_reg_depthR", R.calc_reg_depthR(dr, A["vertices"], temp=2), ("delta_vertices",))
    check("calc_reg_depthC", R.calc_reg_depthC(dr, A["vertices"]), ("delta_vertices",))
    check("calc_reg_deform", R.calc_reg_deform(dr, A["delta_vertices"]), ("delta_vertices",))
    check("recon_flip_L10", R.recon_flip(dr, A, False), ("delta_vertices",))
    assert int(z["recon_flip_L1_raises"]) == 1
    with pytest.raises(RuntimeError):                      # the reference broadcasts (B,V,3)*(B,V) here (networks.py:409)
        R.recon_flip(dr, A, True)
    with pytest.raises(RuntimeError):                      # ... and so does the product, before touching any tensor
        dr.recon_flip(A, True)
    wrt = ("azimuths", "elevations", "distances", "biases", "delta_vertices", "textures", "lights")
    for L1 in (True, False):
        parts = R.recon_att(A, A2, L1=L1, azim=1)
        for nm, val in zip(("cam", "shape", "texture", "light", "bias"), parts):
            check("recon_att_L1%d_%s" % (L1, nm), val, wrt)
    # the mesh regularisers are HIP kernels: host tensors are refused, there is no CPU path
    for call in (lambda: dr.calc_reg_loss(A), lambda: dr.calc_reg_edge(A["vertices"]), lambda: dr.recon_flip(A, False),
                 lambda: dr.recon_att(A, A2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_mesh_reg_tables(pkg):
    """Static tables behind mm_mesh_reg_*: CSR laplacian and its transpose reproduce the dense matrix; adjacency lists invert."""
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "smpl_uv_642.npz"), 32)
    t = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in pkg.mesh_reg.build_tables(dr, torch.device("cpu")).items()}
    V, F, E = dr.num_vertices, dr.num_faces, t["E"]
    L = dr.vertices_laplacian_matrix.numpy()
    for name, M in (("lap", L), ("lapT", L.T)):
        D = np.zeros_like(L)
        for v in range(V):
            s, e = t[name + "_offsets"][v], t[name + "_offsets"][v + 1]
            D[v, t[name + "_cols"][s:e]] = t[name + "_vals"][s:e]
        assert np.array_equal(D, M)
    assert np.allclose(L.sum(1), 0, atol=1e-6) and (np.diag(L) == -1).all()
    for v in range(0, V, 37):
        its = t["ve_items"][t["ve_offsets"][v]:t["ve_offsets"][v + 1]]
        assert all(t["edges"][i >> 1, i & 1] == v for i in its) and len(its) == int((t["edges"] == v).sum())
    for f in range(0, F, 53):
        its = t["fe_items"][t["fe_offsets"][f]:t["fe_offsets"][f + 1]]
        assert all(t["edge2faces"][i >> 1, i & 1] == f for i in its) and len(its) == int((t["edge2faces"] == f).sum())
    for u in range(V):
        its = t["flipT_items"][t["flipT_offsets"][u]:t["flipT_offsets"][u + 1]]
        assert all(t["flip_index"][v] == u for v in its)
    assert t["flipT_offsets"][-1] == V and t["ve_offsets"][-1] == 2 * E and t["fe_offsets"][-1] == 2 * E


def test_deep_copy_and_attributes(pkg):
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "smpl_uv_642.npz"), 64, ratio=2, init_ellipsoid=2)
    assert dr.render_height == 128 and dr.image_size == 64 and dr.num_vertices == 642 and dr.num_faces == 1280
    assert dr.edges.shape == (1920, 2) and dr.edge2faces.shape == (1920, 2) and dr.vertices_laplacian_matrix.shape == (642, 642)
    assert dr.face_uvs.shape == (1, 1280, 3, 2) and dr.uvs.shape[1] == 2 and dr.cam_proj.shape == (3, 1)
    att, _ = pkg.synthetic.synthetic_batch(dr.vertices_init, 3, 128, 64)
    c = pkg.deep_copy(att, index=torch.tensor([2, 0]), detach=True)
    assert set(c) == {"azimuths", "bg", "biases", "elevations", "distances", "vertices", "delta_vertices", "textures", "lights"}
    assert c["vertices"].shape[0] == 2 and torch.equal(c["lights"][0], att["lights"][2])
    att["bg"] = None
    assert pkg.deep_copy(att)["bg"] is None


def test_template_em_update_matches_reference(pkg):
    """template.fuse_template against the reference's inline EM-update statements executed on the same inputs
    (tests/golden/template_em.npz, minted by tests/golden/make_golden_em.py)."""
    z = np.load(os.path.join(GOLDEN, "template_em.npz"))
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), 32)
    av, ad = torch.from_numpy(z["all_vertices"]), torch.from_numpy(z["all_delta_vertices"])
    ran = 0
    for em, smooth, cross, white, count in z["cases"]:
        em, cross, white, count = int(em), int(cross), int(white), int(count)
        tag = "em%d_s%g_c%d_w%d" % (em, smooth, cross, white)
        kw = dict(em=em, smooth=float(smooth), clip=0.05, em_step=0.8, warm_up=0.7, white=bool(white), cross=bool(cross), topK=0.5)
        if count < 0:                                            # the reference itself raises in this mode
            exc = {"IndexError": IndexError, "RuntimeError": RuntimeError}[str(z["raises_" + tag])]
            with pytest.raises(exc):
                pkg.template.fuse_template(dr.vertices_init, dr.vertices_laplacian_matrix, av, ad, **kw)
            continue
        new, n, _ = pkg.template.fuse_template(dr.vertices_init, dr.vertices_laplacian_matrix, av, ad, **kw)
        assert n == count and new.shape == (1, dr.num_vertices, 3)
        np.testing.assert_allclose(new.numpy(), z["new_" + tag], rtol=0, atol=2e-7)
        ran += 1
    assert ran >= 9
    # the update moved the template, stayed within the clip, and the cross rule can veto it
    moved = np.abs(z["new_em1_s0_c0_w0"] - dr.vertices_init.numpy()[None]).max()
    assert 0 < moved <= 0.7 * 0.8 * 0.05 + 1e-7


def test_next_row_entry_points_validate_before_any_gpu_work(pkg):
    """mm_mesh_reg_*, mm_attribute_loss_*, mm_texture_flow_*: argument validation happens on the host (no GPU here)."""
    N = pkg._native
    L = N.lib()
    d = N.MMMeshRegDesc()
    assert L.mm_mesh_reg_forward(ctypes.byref(d), None) == -2                       # MM_ERR_BAD_SHAPE
    d.B, d.V, d.F, d.E, d.terms = 2, 10, 12, 20, 1 << 3
    assert L.mm_mesh_reg_query_workspace(ctypes.byref(d)) % 256 == 0 and L.mm_mesh_reg_query_workspace(ctypes.byref(d)) > 0
    assert L.mm_mesh_reg_forward(ctypes.byref(d), None) == -1                       # DEPTH needs vertices
    d.terms = 1 << 9
    assert L.mm_mesh_reg_forward(ctypes.byref(d), None) == -2
    a = N.MMAttLossDesc()
    assert L.mm_attribute_loss_forward(ctypes.byref(a), None) == -2
    a.B, a.V, a.Ht, a.Wt = 2, 10, 8, 4
    assert L.mm_attribute_loss_query_workspace(ctypes.byref(a)) % 256 == 0
    assert L.mm_attribute_loss_forward(ctypes.byref(a), None) == -1
    t = N.MMTexFlowDesc()
    assert L.mm_texture_flow_forward(ctypes.byref(t), None) == -2
    t.B, t.C, t.H, t.W, t.Ho, t.Wo = 1, 3, 8, 8, 8, 8
    assert L.mm_texture_flow_forward(ctypes.byref(t), None) == -1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.sample_texture(torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8))


def test_chamfer_entry_points_validate_before_any_gpu_work(pkg):
    """mm_nearest_neighbour, mm_chamfer_nearest and mm_chamfer_backward refuse null pointers, empty or negative sizes and a batch
    beyond the grid's y limit (B > 65535) on the host, with their status and before any launch (host buffers stand in for device
    pointers: none of them may reach a kernel)."""
    N = pkg._native
    L = N.lib()
    fb = (ctypes.c_float * 64)()
    ib = (ctypes.c_int32 * 64)()
    f, i = ctypes.cast(fb, ctypes.c_void_p), ctypes.cast(ib, ctypes.c_void_p)

    def calls(B, Nn, M, null=None):
        def p(k, v):
            return None if k == null else v
        return {
            "mm_nearest_neighbour": lambda: L.mm_nearest_neighbour(B, Nn, M, p(0, f), p(1, f), p(2, f), p(3, i), None),
            "mm_chamfer_nearest": lambda: L.mm_chamfer_nearest(B, Nn, M, p(0, f), p(1, f), p(2, f), p(3, i), p(4, f), p(5, i), None),
            "mm_chamfer_backward": lambda: L.mm_chamfer_backward(B, Nn, M, p(0, f), p(1, f), p(2, i), p(3, i), p(4, f), p(5, f), p(6, f), None),
        }
    nptr = {"mm_nearest_neighbour": 4, "mm_chamfer_nearest": 6, "mm_chamfer_backward": 7}
    for name, n in nptr.items():
        for k in range(n):
            assert calls(2, 9, 9, null=k)[name]() == -1, (name, k)                  # MM_ERR_NULL_POINTER
        assert calls(0, 0, 0, null=0)[name]() == -1, name                           # (pointers are checked first)
        for B, Nn, M in ((0, 9, 9), (2, 0, 9), (2, 9, 0), (-1, 9, 9), (2, -5, 9), (2, 9, -5)):
            assert calls(B, Nn, M)[name]() == -2, (name, B, Nn, M)                  # MM_ERR_BAD_SHAPE
        assert calls(65536, 9, 9)[name]() == -5, name                               # MM_ERR_UNSUPPORTED: batch rows are grid y
        assert calls(1 << 20, 1, 1)[name]() == -5, name
    assert L.mm_last_error_detail().decode() == ""                                  # nothing was launched
    assert "mm_chamfer_backward" in N.EXPORTS


def test_workspace_query_and_status_validation(pkg):
    """The render workspace is right-sized (round 3: the texture-gradient records are packed per image, no per-tile capacities) and
    mm_render_status validates its arguments on the host before it touches the device."""
    N = pkg._native
    L = N.lib()
    d = N.MMRenderDesc()
    assert L.mm_query_workspace(ctypes.byref(d)) == 0
    assert L.mm_render_status(None, None, None) == -1                                # MM_ERR_NULL_POINTER
    assert L.mm_render_status(ctypes.byref(d), None, None) == -2                     # MM_ERR_BAD_SHAPE
    d.B, d.H, d.W, d.V, d.F, d.Ht, d.Wt = 48, 128, 128, 642, 1280, 256, 128          # BASELINE config 2
    n2 = L.mm_query_workspace(ctypes.byref(d))
    assert n2 % 256 == 0 and 40e6 < n2 < 80e6                                        # 301 MB in round 2
    assert L.mm_render_status(ctypes.byref(d), None, None) == -1                     # no workspace
    d.B, d.H, d.W, d.V, d.F, d.Ht, d.Wt = 16, 512, 512, 6890, 13776, 1024, 512       # config 5
    n5 = L.mm_query_workspace(ctypes.byref(d))
    assert 300e6 < n5 < 400e6                                                        # 1 007 MB in round 2
    dr = pkg.DiffRender(os.path.join(TEMPLATES, "sphere.npz"), 64)
    d.B, d.H, d.W, d.V, d.F, d.Ht, d.Wt = 2, 64, 64, dr.num_vertices, dr.num_faces, 64, 64
    base = dr.workspace_bytes(d)
    dr.extra_texture_records_per_pixel = 1.5
    assert dr.workspace_bytes(d) == base + 2 * int(1.5 * 64 * 64) * 24                 # 24-byte records, per image
