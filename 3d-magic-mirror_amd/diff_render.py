"""Host-side mirror of the reference's ``DiffRender`` (/root/reference/networks.py:164-491) over the gfx950 C ABI.

Same constructor, attributes, method names, argument meaning and return values as the reference class, so a
``trainer.py``-style loop can switch with ``from mm_amd import DiffRender``.  ``render``, ``render_views``, ``render_indexed``, ``render_geometry``, ``render_recon``
and ``recon_data`` run the hand-written HIP kernels of ``lib/libmm_render.so`` through the C++ autograd nodes of
``lib/mm_torch_ext.so`` (csrc/mm_torch_ext.cpp); there is no CPU, eager-torch or Python-node fallback for them.  The mesh
regularisers (``recon_flip``, ``calc_reg_*``) run as one HIP launch per direction (``mesh_reg.py``), and so
do the attribute losses of ``recon_att`` (``att_loss.py``); its chamfer term is a HIP nearest-neighbour kernel.
"""
import ctypes

import numpy as np
import torch

from . import _native as N
from . import att_loss, mesh_reg, obj_io, template


class _SplitBatchFn(torch.autograd.Function):
    """x (sum(sizes), ...) -> its per-set pieces along the batch, with a backward that CONCATENATES the pieces' gradients (one copy per piece
    into one buffer).  Plain slicing would have autograd build, per piece, a full-size zero tensor with the piece filled in and then add
    them up: three fills and two adds of the whole batched image where one write per piece suffices (render_many)."""

    @staticmethod
    def forward(ctx, x, *sizes):
        ctx.sizes, ctx.shape = sizes, tuple(x.shape)
        ctx.set_materialize_grads(False)
        out, o = [], 0
        for n in sizes:
            out.append(x.narrow(0, o, n))
            o += n
        return tuple(out)

    @staticmethod
    def backward(ctx, *grads):
        if all(g is None for g in grads):
            return (None,) * (1 + len(ctx.sizes))
        ref = next(g for g in grads if g is not None)
        full = torch.empty(ctx.shape, device=ref.device, dtype=ref.dtype)
        o = 0
        for n, g in zip(ctx.sizes, grads):
            if g is None:
                full.narrow(0, o, n).zero_()
            else:
                full.narrow(0, o, n).copy_(g)
            o += n
        return (full,) + (None,) * len(ctx.sizes)


INDEXED = ('vertices', 'textures', 'lights', 'bg')             # the tensors a render_indexed image picks a row of, in the C ABI's order


def grid_index(n_rows, n_cols):
    """(row_of_image, col_of_image), two (n_rows * n_cols,) int64 CPU tensors, for the images of a row-major grid: image i sits in row
    i // n_cols, column i % n_cols.  The rainbow sheet of show_rainbow2.py:376-399 (a row per texture, a column per shape) is
    ``row, col = grid_index(n_textures, n_shapes)`` and ``index={"vertices": col, "lights": col, "textures": row}``."""
    n_rows, n_cols = int(n_rows), int(n_cols)
    if n_rows < 1 or n_cols < 1:
        raise ValueError("grid_index needs at least one row and one column, got %d x %d" % (n_rows, n_cols))
    i = torch.arange(n_rows * n_cols, dtype=torch.int64)
    return torch.div(i, n_cols, rounding_mode="floor"), i % n_cols


def check_render_index(index, rows, M):
    """The `index` argument of render_indexed against the row counts `rows` ({name: R}, the call's tensors) and the image count M, on the
    host: {name: None (the identity) | a device tensor as given (NOT validated: the plan kernel does that) | a validated (M,) int64 CPU tensor}.
    ValueError for an unknown name, an identity over a tensor that does not hold M rows, a wrong length or an out-of-range host entry."""
    index = dict(index or {})
    for k in index:
        if k not in INDEXED:
            raise ValueError("render_indexed: index has no %r (the indexed tensors are %s)" % (k, ", ".join(INDEXED)))
    out = {}
    for k, R in rows.items():
        v = index.get(k)
        if v is None:
            if R != M:
                raise ValueError("render_indexed: %s holds %d rows for %d images and index[%r] is missing (a missing index is the identity)" % (k, R, M, k))
            out[k] = None
            continue
        if torch.is_tensor(v) and v.device.type != "cpu":
            if v.dim() != 1 or v.shape[0] != M or v.dtype not in (torch.int32, torch.int64):
                raise ValueError("render_indexed: index[%r] must be an (%d,) int32 or int64 tensor, got %s %s" % (k, M, tuple(v.shape), v.dtype))
            out[k] = v
            continue
        t = torch.as_tensor(np.asarray(v.detach().numpy() if torch.is_tensor(v) else v))
        if t.dtype in (torch.float16, torch.float32, torch.float64, torch.bool) or t.is_complex():
            raise ValueError("render_indexed: index[%r] must hold integers, got %s" % (k, t.dtype))
        t = t.to(torch.int64)
        if t.dim() != 1 or t.shape[0] != M:
            raise ValueError("render_indexed: index[%r] must hold %d entries, one per image; got shape %s" % (k, M, tuple(t.shape)))
        if M and (int(t.min()) < 0 or int(t.max()) >= R):
            bad = int(((t < 0) | (t >= R)).nonzero()[0])
            raise ValueError("render_indexed: index[%r][%d] = %d is outside the %d rows of %s" % (k, bad, int(t[bad]), R, k))
        out[k] = t
    return out


def require_tensors(who, attributes):
    """TypeError unless the seven attributes every render reads are tensors (`who`: the calling method, for the message)."""
    for k in ('vertices', 'textures', 'lights', 'azimuths', 'elevations', 'distances', 'biases'):
        if not torch.is_tensor(attributes.get(k)):
            raise TypeError("%s needs attributes[%r] as a tensor" % (who, k))


def sub_desc(cls, proto, **fields):
    """A multi-view or indexed descriptor: the render prototype's bytes, then the fields of its own."""
    vd = cls()
    ctypes.memmove(ctypes.byref(vd), proto, len(proto))
    for k, v in fields.items():
        setattr(vd, k, v)
    return vd


class DiffRender(object):
    """Drop-in for ``networks.DiffRender`` (networks.py:164)."""

    def __init__(self, mesh_name, image_size, ratio=1, init_ellipsoid=1, image_weight=0.1, lambda_lpl=0.1, lambda_flat=0.001,
                 emit_imnormal=True, verbose=False):
        self.image_size = image_size
        self.image_weight = image_weight
        self.lambda_lpl = lambda_lpl
        self.lambda_flat = lambda_flat
        self.ratio = ratio
        self.emit_imnormal = emit_imnormal
        self.options = 0                                # MMRenderDesc.options: MM_OPT_* bits (SURVEY Appendix C switches); 0 = defaults
        # The render workspace is the library's minimum (mm_query_workspace) plus room for this many MORE texture-gradient records per pixel
        # than the 9/8 the minimum holds (include/mm_render.h); an image that runs out gets NaN texture gradients, and with
        # check_texture_records every render backward of the class API (RenderNode, deferred or not) asks the library (a stream synchronisation)
        # and raises instead.
        self.extra_texture_records_per_pixel = 0.0
        self.check_texture_records = False
        # DEFERRED FUSION (csrc/mm_torch_ext.cpp, MMRenderDesc.fused_totals): `recon_data(pred, gt)` on the untouched image of an earlier
        # `render` of this process -- the un-modified trainer's order of calls (trainer.py:276,441) -- forms its value as always and routes its BACKWARD
        # through the render node: no dL/d image tensor, no loss-backward launch; every gradient of the render's inputs has the bits of the two separate
        # backward passes.  The one observable difference: recon_data's contribution to the gradient OF THE IMAGE ITSELF (torch.autograd.grad(loss, rgbs),
        # a hook on rgbs, rgbs.retain_grad()) does not exist as a tensor -- set this to False if the image's own gradient is inspected.
        self.defer_recon_fusion = True
        camera_fovy = np.arctan(1.0 / 2.5) * 2
        self.cam_proj = template.generate_perspective_projection(camera_fovy, ratio=1 / ratio)     # networks.py:172-174
        mesh = obj_io.load_template(mesh_name)                                                   # :176
        self.vertices_init = template.normalize_template(mesh.vertices, init_ellipsoid)          # :181-194
        self.faces = mesh.faces
        self.uvs = mesh.uvs
        self.face_uvs = template.index_vertices_by_faces(mesh.uvs.unsqueeze(0), mesh.face_uvs_idx).detach()  # :196-202
        self.num_faces = self.faces.shape[0]
        self.num_vertices = self.vertices_init.shape[0]
        self.flip_index = template.flip_pairing(self.vertices_init)                              # :215-217
        self.edges, self.edge2faces = template.edge_tables(self.faces)                           # :220-246
        self.vertices_laplacian_matrix = template.uniform_laplacian(self.num_vertices, self.faces)  # :249
        self.sign_init = torch.sign(self.vertices_init[:, 2])                                    # :252 (device copy made lazily)
        if torch.cuda.is_available():
            self.sign_init = self.sign_init.cuda()
        self.render_height = round(self.ratio * self.image_size)                                  # :298
        self._vc_table = template.vertex_corner_table(self.num_vertices, self.faces)     # (V, stride, 4): the backward's vertex -> corner gather
        self._static_cache = {}
        self._desc_cache = {}
        self._status = None                                      # one pinned int32 the backward kernels add dropped-record counts to (MMRenderDesc.status_flag)
        # dibr_rasterization defaults (kaolin v0.12.0): sigmainv=7000, boxlen=0.02, knum=30, multiplier=1000, eps=1e-8
        self.sigmainv, self.boxlen, self.knum, self.multiplier, self.eps = 7000.0, 0.02, 30, 1000.0, 1e-8
        if verbose:
            print("Vertices Number:", self.num_vertices)
            print("Faces Number:", self.faces.shape)
            print("Unique Edge Number: %d" % self.edges.shape[0])

    # ---- device-resident static template data (the reference re-uploads faces/face_uvs on every call, :272-273) ----
    def _static(self, device):
        """The template's faces, face uvs and vertex-corner table on ``device``, made once per device.  Resident: each upload is a blocking
        copy from pageable memory that has finished when this returns, and the tensors are only read afterwards, so calls on any stream
        may share them."""
        key = str(device)
        st = self._static_cache.get(key)
        if st is None:
            st = {"faces": self.faces.to(device=device, dtype=torch.int32).contiguous(),
                  "face_uvs": self.face_uvs.to(device=device, dtype=torch.float32).reshape(-1, 3, 2).contiguous(),
                  "vc_table": self._vc_table.to(device=device, dtype=torch.int32).contiguous()}
            self._static_cache[key] = st
        return st

    def _render_node(self, no_mask, gt, vertices, textures, lights, bg, azimuths, elevations, distances, biases, contour=0.0):
        """One C++ autograd node for the render, + the fused loss if gt is given (csrc/mm_torch_ext.cpp: RenderNode; no Python in the backward).
        With check_texture_records, its backward also asks mm_render_status and raises if texture-gradient records were dropped."""
        self._raise_if_records_were_dropped()                    # (an overflow of an EARLIER step's backward: a host read of pinned memory, no sync)
        N.require_device(azimuths)
        if no_mask and bg is None:
            raise TypeError("render(no_mask=True) needs attributes['bg'] (B,3,H,W)")   # reference: None.permute fails
        if textures.dim() != 4:
            raise RuntimeError("textures must be (B,3,Ht,Wt), got %s" % (tuple(textures.shape),))
        dev = azimuths.device
        proto, nbytes = self._proto(self._static(dev), azimuths.numel(), no_mask, textures.shape[2], textures.shape[3], float(contour) if gt is not None else 0.0)
        return N.torch_ext().render(N.fn_addr("mm_render_forward"), N.fn_addr("mm_render_fused_loss"), N.fn_addr("mm_render_backward"),
                                    N.fn_addr("mm_render_status") if self.check_texture_records else 0, proto, nbytes,
                                    vertices, textures, lights, bg, azimuths, elevations, distances, biases, gt, bool(self.emit_imnormal),
                                    float(self.image_weight), bool(self.defer_recon_fusion))

    def _status_ptr(self):
        """Address of this object's pinned status word (device-writable host memory): every descriptor built here carries it, so that a
        backward that drops texture-gradient records -- eager, C++ node or captured graph -- is noticed WITHOUT a synchronisation."""
        if self._status is None:
            self._status = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._status_word = ctypes.c_int32.from_address(self._status.data_ptr())     # (a plain host read per poll: ~0.1 us)
        return self._status.data_ptr()

    def poll_dropped_records(self, reset=True):
        """Texture-gradient records dropped by backward passes that have COMPLETED since the last poll (no synchronisation: a host read)."""
        if self._status is None:
            return 0
        n = self._status_word.value
        if n and reset:
            self._status_word.value = 0
        return n

    def _raise_if_records_were_dropped(self):
        n = self.poll_dropped_records()
        if n:
            raise RuntimeError("an earlier call of this DiffRender added %d to its status word.  Two things count there and cannot be told apart "
                               "afterwards: (1) a backward dropped that many texture-gradient records (record pool overflow; the texture gradients of the "
                               "affected images were NaN: raise DiffRender.extra_texture_records_per_pixel), or (2) a render_indexed call found that many "
                               "entries of a device index outside their tensor's rows (those images are NaN with face_idx -1 and take no part in "
                               "any gradient: check the index tensors)." % n)

    def workspace_bytes(self, d):
        """Bytes of the render workspace for the shape in MMRenderDesc `d`: the library's minimum + the extra record pool asked for."""
        extra = int(np.ceil(max(0.0, float(self.extra_texture_records_per_pixel)) * d.H * d.W)) * 24 * d.B
        return int(N.lib().mm_query_workspace(ctypes.byref(d))) + extra

    def _prototype(self, st, B, no_mask, Ht, Wt, contour=0.0, geometry_only=False):
        """(MMRenderDesc prototype of this shape, its bytes, its workspace size), filled once per shape and cached: sizes, dibr constants,
        template pointers, options and the status word -- everything of a descriptor but the per-call tensor pointers."""
        key = (id(st), B, int(bool(no_mask)), Ht, Wt, self.knum, self.sigmainv, self.boxlen, self.multiplier, self.eps, self.options,
               float(self.extra_texture_records_per_pixel), float(contour), bool(geometry_only))
        hit = self._desc_cache.get(key)
        if hit is None:
            d = N.MMRenderDesc()
            d.geometry_only = 1 if geometry_only else 0
            d.B, d.H, d.W, d.V, d.F = B, self.render_height, self.image_size, self.num_vertices, self.num_faces
            d.Ht, d.Wt = Ht, Wt
            d.no_mask, d.knum = int(bool(no_mask)), self.knum
            for i in range(3):
                d.proj[i] = float(self.cam_proj[i, 0])
            d.sigmainv, d.boxlen, d.multiplier, d.eps = self.sigmainv, self.boxlen, self.multiplier, self.eps
            d.faces, d.face_uvs = N.ptr(st["faces"]), N.ptr(st["face_uvs"])
            d.vc_table, d.vc_stride = N.ptr(st["vc_table"]), int(st["vc_table"].shape[1])
            d.options = self.options
            d.status_flag = self._status_ptr()
            d.fused_contour = float(contour)
            hit = (d, bytes(d), self.workspace_bytes(d))
            if len(self._desc_cache) > 32:
                self._desc_cache.clear()
            self._desc_cache[key] = hit
        return hit

    def _proto(self, st, B, no_mask, Ht, Wt, contour=0.0, geometry_only=False):
        """(bytes of the MMRenderDesc prototype of this shape, its workspace size) for the C++ nodes, which copy the prototype for their
        forward AND their backward -- so contour (MMRenderDesc.fused_contour) travels in it."""
        return self._prototype(st, B, no_mask, Ht, Wt, contour, geometry_only)[1:]

    def _desc(self, st, B, no_mask, vertices, textures, lights, bg, azimuths, elevations, distances, biases, rgba, face_idx, fn, imn):
        """MMRenderDesc for one call (step.RenderLossStep): a copy of the shape's prototype with the per-call pointers set."""
        d = N.MMRenderDesc.from_buffer_copy(self._prototype(st, B, no_mask, textures.shape[2], textures.shape[3])[0])
        dp = lambda t: None if t is None else t.data_ptr()
        d.vertices, d.textures, d.lights, d.bg = dp(vertices), dp(textures), dp(lights), dp(bg)
        d.azimuths, d.elevations, d.distances, d.biases = dp(azimuths), dp(elevations), dp(distances), dp(biases)
        d.rgba, d.face_idx, d.face_normals, d.imnormal = dp(rgba), dp(face_idx), dp(fn), dp(imn)
        return d

    def _set_outputs(self, attributes, fn, imn, face_idx):
        """What every render leaves beside its image: the two attributes networks.py:319-320 sets, and the face index map."""
        attributes['face_normals'] = fn
        attributes['imnormal'] = imn if self.emit_imnormal else None
        self.last_face_idx = face_idx                   # kaolin returns it from dibr_rasterization; the reference drops it

    # ---- networks.py:258-324 -------------------------------------------------------------------------------------
    def render(self, no_mask=False, **attributes):
        azimuths = attributes['azimuths']
        elevations = attributes['elevations']
        distances = attributes['distances']
        biases = attributes['biases']
        bg = attributes['bg']
        vertices = attributes['vertices']
        textures = attributes['textures']
        lights = attributes['lights']
        rgba, fn, imn, face_idx = self._render_node(bool(no_mask), None, vertices, textures, lights, bg if no_mask else None,
                                                    azimuths, elevations, distances, biases)
        self._set_outputs(attributes, fn, imn, face_idx)
        return rgba.permute(0, 3, 1, 2), attributes     # (B,4,H,W) view of NHWC memory, like networks.py:317

    # ---- the same samples under several cameras (trainer.py:280-289,347 Ae / Ae90; :710-723 evaluation; :619-671 turntables) ----
    def _view_cameras(self, attributes):
        """(B, N, the four camera attributes as (B,N) / (B,N,2)) of a render_views call, every shape checked: B from `vertices`; a camera
        attribute is (B,N) (biases (B,N,2)) or, broadcast over the views, (B,) (biases (B,2)); at least one carries N and all that do agree."""
        require_tensors("render_views", attributes)
        vertices, textures, lights = attributes['vertices'], attributes['textures'], attributes['lights']
        if vertices.dim() != 3 or tuple(vertices.shape[1:]) != (self.num_vertices, 3):
            raise ValueError("vertices must be (B,%d,3), got %s" % (self.num_vertices, tuple(vertices.shape)))
        B = int(vertices.shape[0])
        if textures.dim() != 4 or textures.shape[0] != B or textures.shape[1] != 3:
            raise ValueError("textures must be (%d,3,Ht,Wt) -- one per SAMPLE, not per view -- got %s" % (B, tuple(textures.shape)))
        if tuple(lights.shape) != (B, 9):
            raise ValueError("lights must be (%d,9) -- one row per SAMPLE, not per view -- got %s" % (B, tuple(lights.shape)))
        shapes = {k: tuple(attributes[k].shape) for k in ('azimuths', 'elevations', 'distances', 'biases')}
        views = {}
        for k, shp in shapes.items():
            tail = (2,) if k == 'biases' else ()
            if shp == (B,) + tail:
                continue                                          # broadcast over the views
            if len(shp) == 2 + len(tail) and shp[0] == B and shp[1] >= 1 and shp[2:] == tail:
                views[k] = shp[1]
            else:
                raise ValueError("%s must be (%d,N%s) or, the same for every view, (%d%s); got %s (camera shapes: %s)"
                                 % (k, B, ",2" if tail else "", B, ",2" if tail else ",", shp, shapes))
        if not views:
            raise ValueError("render_views: no camera attribute carries a view axis -- give at least one of azimuths / elevations / distances as "
                             "(%d,N) or biases as (%d,N,2) (got %s); for one view per sample call render" % (B, B, shapes))
        if len(set(views.values())) != 1:
            raise ValueError("render_views: the camera attributes disagree on the number of views: %s" % views)
        n = next(iter(views.values()))
        cams = []
        for k in ('azimuths', 'elevations', 'distances', 'biases'):
            t = attributes[k]
            cams.append(t if k in views else t.unsqueeze(1).expand((B, n) + tuple(t.shape[1:])))
        return B, n, cams

    def render_views(self, no_mask=False, **attributes):
        """``render`` of B samples under N cameras each, as ONE pass of the kernels over B*N images in which every sample's vertices, textures,
        lights and bg are read from their single (B,...) copy -- nothing is replicated per view on the way in, at any layer (csrc/mm_torch_ext.cpp:
        RenderViewsNode; include/mm_render.h: MMRenderViewsDesc).  Camera attributes are (B,N) (biases (B,N,2)); one given as (B,) / (B,2) holds for
        every view (a turntable passes azimuths (B,36) and leaves the rest alone) and receives its gradient through autograd's expand.
        Returns (rgbs (B,N,4,H,W) -- the permuted view of (B,N,H,W,4) memory, like render's --, attributes) with attributes['face_normals']
        (B,N,F,3), attributes['imnormal'] (B,N,H,W,3) or None, and self.last_face_idx (B,N,H,W).  Image (b,n) is bit-identical to image b*N + n of
        ``render`` on the per-sample tensors replicated with repeat_interleave(N, 0); the gradient of a per-sample tensor is the fp32 sum of its
        views' gradients in ascending view order (plain adds: bitwise reproducible)."""
        no_mask = bool(no_mask)
        if no_mask and attributes.get('bg') is None:
            raise TypeError("render_views(no_mask=True) needs attributes['bg'] (B,3,H,W)")
        B, n, (azimuths, elevations, distances, biases) = self._view_cameras(attributes)
        vertices, textures, lights = attributes['vertices'], attributes['textures'], attributes['lights']
        bg = attributes['bg'] if no_mask else None
        if bg is not None and tuple(bg.shape) != (B, 3, self.render_height, self.image_size):
            raise ValueError("bg must be (%d,3,%d,%d) -- one per SAMPLE, not per view -- got %s" % (B, self.render_height, self.image_size, tuple(bg.shape)))
        self._raise_if_records_were_dropped()
        N.require_device(azimuths, elevations, distances, biases, vertices, textures, lights, bg)
        st = self._static(azimuths.device)
        Ht, Wt = int(textures.shape[2]), int(textures.shape[3])
        proto, nbytes = self._proto(st, B * n, no_mask, Ht, Wt)
        # the workspace's head; the B*N images' render workspace (render's own size) follows
        staging = self._head_bytes(("views", proto, n), lambda: sub_desc(N.MMRenderViewsDesc, proto, views=n),
                                   "mm_render_views_query_workspace", lambda: "%d views" % n)
        rgba, fn, imn, face_idx = N.torch_ext().render_views(
            N.fn_addr("mm_render_views_forward"), N.fn_addr("mm_render_views_backward"),
            N.fn_addr("mm_render_status") if self.check_texture_records else 0, proto, n, nbytes + staging, staging,
            vertices, textures, lights, bg, azimuths, elevations, distances, biases, bool(self.emit_imnormal))
        self._set_outputs(attributes, fn, imn, face_idx)
        return rgba.permute(0, 1, 4, 2, 3), attributes

    def _head_bytes(self, key, make_desc, query, shape):
        """What a multi-view or indexed workspace holds in front of the render workspace of its images (render_views: the staging areas of the
        per-image gradients; render_indexed: the plan and, for a call with a backward, the staging areas), cached under `key`: the library's
        `query` (its name) of the sub-descriptor make_desc() minus mm_query_workspace of its render.  shape(): the refusal's words for the shape."""
        hit = self._desc_cache.get(key)
        if hit is None:
            vd = make_desc()
            hit = int(getattr(N.lib(), query)(ctypes.byref(vd))) - int(N.lib().mm_query_workspace(ctypes.byref(vd.render)))
            if hit < 0:
                raise RuntimeError("%s refused the shape (%d images, %s)" % (query, vd.render.B, shape()))
            self._desc_cache[key] = hit
        return hit

    # ---- every image picks its rows (show_rainbow2.py:376-399 the rainbow sheets; networks.py:146-161 deep_copy(index=...) + render) ----
    def render_indexed(self, no_mask=False, index=None, **attributes):
        """``render`` of M images, each of which reads the row of ``vertices``, ``textures``, ``lights`` and ``bg`` that ``index`` names for it, as ONE
        pass of the kernels -- nothing is gathered on the way in (csrc/mm_torch_ext.cpp: RenderIndexedNode; include/mm_render.h: MMRenderIndexedDesc).
        The cameras are per image, (M,) / biases (M,2); the four indexed tensors carry row counts of their own.  ``index`` is a dict with any of
        those four names; a missing name is the identity, and that tensor then needs M rows.  A value is a device tensor (int32 or int64:
        converted on the device, NOT validated on the host -- an entry out of range makes its image NaN with face_idx -1, leaves it out of every
        gradient sum, and raises on this object's next call) or a CPU tensor, list or numpy array (validated here with ValueError, then uploaded).
        Returns (rgbs (M,4,H,W) -- the usual permuted view of NHWC memory --, attributes) with attributes['face_normals'] (M,F,3),
        attributes['imnormal'] and self.last_face_idx (M,H,W).  Image i is bit-identical to image i of ``render`` on the tensors gathered with
        index_select; the gradient of an indexed tensor has the tensor's own shape: row r's is the fp32 sum of the gradients of the images that
        read it, in ascending image order (plain adds: bitwise reproducible), zeros for a row no image reads.
        Not here: blending two rows inside the render (``mix_attributes``), the fused loss and step mode over indices."""
        no_mask = bool(no_mask)
        require_tensors("render_indexed", attributes)
        if no_mask and not torch.is_tensor(attributes.get('bg')):
            raise TypeError("render_indexed(no_mask=True) needs attributes['bg'] (R,3,H,W)")
        azimuths, elevations, distances, biases = (attributes[k] for k in ('azimuths', 'elevations', 'distances', 'biases'))
        vertices, textures, lights = attributes['vertices'], attributes['textures'], attributes['lights']
        bg = attributes['bg'] if no_mask else None
        M = int(azimuths.numel())
        if M < 1 or any(int(t.numel()) != M for t in (elevations, distances)) or int(biases.numel()) != 2 * M or biases.shape[-1] != 2:
            raise ValueError("render_indexed: the cameras must hold one value per image (biases a pair): got azimuths %s, elevations %s, distances %s, "
                             "biases %s" % tuple(tuple(t.shape) for t in (azimuths, elevations, distances, biases)))
        if vertices.dim() != 3 or tuple(vertices.shape[1:]) != (self.num_vertices, 3) or vertices.shape[0] < 1:
            raise ValueError("vertices must be (R,%d,3), got %s" % (self.num_vertices, tuple(vertices.shape)))
        if textures.dim() != 4 or textures.shape[1] != 3 or textures.shape[0] < 1:
            raise ValueError("textures must be (R,3,Ht,Wt), got %s" % (tuple(textures.shape),))
        if lights.dim() != 2 or lights.shape[1] != 9 or lights.shape[0] < 1:
            raise ValueError("lights must be (R,9), got %s" % (tuple(lights.shape),))
        if bg is not None and (bg.dim() != 4 or tuple(bg.shape[1:]) != (3, self.render_height, self.image_size) or bg.shape[0] < 1):
            raise ValueError("bg must be (R,3,%d,%d), got %s" % (self.render_height, self.image_size, tuple(bg.shape)))
        rows = {'vertices': int(vertices.shape[0]), 'textures': int(textures.shape[0]), 'lights': int(lights.shape[0])}
        if bg is not None:
            rows['bg'] = int(bg.shape[0])
        if M > 65535 or max(rows.values()) > 65535:
            raise ValueError("render_indexed takes at most 65535 images and 65535 rows per tensor (got %d images, rows %s)" % (M, rows))
        idx = check_render_index(index, rows, M)
        self._raise_if_records_were_dropped()
        N.require_device(azimuths, elevations, distances, biases, vertices, textures, lights, bg)
        dev = azimuths.device
        idx = {k: (None if v is None else v.to(device=dev, dtype=torch.int32).contiguous()) for k, v in idx.items()}
        N.require_device(*[v for v in idx.values() if v is not None])
        st = self._static(dev)
        Ht, Wt = int(textures.shape[2]), int(textures.shape[3])
        proto, nbytes = self._proto(st, M, no_mask, Ht, Wt)
        backward = torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                                   for t in (vertices, textures, lights, bg, azimuths, elevations, distances, biases))
        nrows = tuple(rows.get(k, M) for k in INDEXED)
        head = self._head_bytes(("indexed", proto, nrows, bool(backward)),
                                lambda: sub_desc(N.MMRenderIndexedDesc, proto, rows=nrows, backward=1 if backward else 0),
                                "mm_render_indexed_query_workspace", lambda: "rows %s" % (nrows,))
        self.last_indexed_workspace_bytes = nbytes + head         # (what the node allocates: the forward-only query when nothing requires grad)
        rgba, fn, imn, face_idx = N.torch_ext().render_indexed(
            N.fn_addr("mm_render_indexed_forward"), N.fn_addr("mm_render_indexed_backward"),
            N.fn_addr("mm_render_status") if self.check_texture_records else 0, proto, nbytes + head, head, self._status_ptr(), bool(backward),
            vertices, textures, lights, bg, azimuths, elevations, distances, biases, idx['vertices'], idx['textures'], idx['lights'], idx.get('bg'),
            bool(self.emit_imnormal))
        self._set_outputs(attributes, fn, imn, face_idx)
        return rgba.permute(0, 3, 1, 2), attributes

    def render_many(self, attribute_sets, no_mask=False):
        """Several INDEPENDENT ``render`` calls as one: the attribute sets (same shapes) are concatenated along the batch and rendered by ONE pass
        of the kernels over sum(B) images -- the renders of trainer.py:276, :345 and :347 all exist as attributes before any of them runs, and
        three launches-bound passes of 48 images cost more than one of 144.  Returns [(rgbs, attributes), ...] like the separate calls would:
        per-set views of the batched outputs; gradients flow back through the concatenation into every set's own tensors.
        Results per image are those of the separate calls bit for bit (an image's render does not depend on its batch)."""
        sets = list(attribute_sets)
        if not sets:
            return []
        keys = ('vertices', 'textures', 'lights', 'azimuths', 'elevations', 'distances', 'biases') + (('bg',) if no_mask else ())
        sizes = [int(a['azimuths'].reshape(-1).shape[0]) for a in sets]
        cat = {k: (sets[0][k] if len(sets) == 1 else torch.cat([a[k].reshape((n,) + tuple(a[k].shape[1:]) if a[k].dim() > 1 else (n,)) for a, n in zip(sets, sizes)], 0))
               for k in keys}
        rgba, fn, imn, face_idx = self._render_node(bool(no_mask), None, cat['vertices'], cat['textures'], cat['lights'], cat.get('bg'),
                                                    cat['azimuths'], cat['elevations'], cat['distances'], cat['biases'])
        rgba_p = _SplitBatchFn.apply(rgba, *sizes) if len(sets) > 1 else (rgba,)
        fn_p = _SplitBatchFn.apply(fn, *sizes) if len(sets) > 1 else (fn,)
        out, o = [], 0
        for a, n, r, f in zip(sets, sizes, rgba_p, fn_p):
            self._set_outputs(a, f, imn[o:o + n], face_idx)       # (last_face_idx: the whole batch's)
            out.append((r.permute(0, 3, 1, 2), a))
            o += n
        return out

    def render_geometry(self, **attributes):
        """``render`` for the call site that throws the image away (trainer.py:367: ``_, Aire = diffRender.render(**Aire)`` keeps only
        ``attributes['face_normals']``): the vertex stage alone -- camera, prepare_vertices, face normals -- with its backward to vertices and
        camera; nothing is rasterised, shaded or stored.  Returns the attributes with 'face_normals' set (bit-identical to render's) and
        'imnormal' None."""
        a = attributes
        self._raise_if_records_were_dropped()
        N.require_device(a['azimuths'])
        dev = a['azimuths'].device
        tex = a['textures']
        proto, nbytes = self._proto(self._static(dev), a['azimuths'].numel(), False, tex.shape[2], tex.shape[3], 0.0, geometry_only=True)
        # (the C++ node, csrc/mm_torch_ext.cpp: GeometryNode; it writes no texture records, so check_texture_records has nothing to ask)
        attributes['face_normals'] = N.torch_ext().render_geometry(N.fn_addr("mm_render_forward"), N.fn_addr("mm_render_backward"), proto, nbytes,
                                                                   a['vertices'], a['azimuths'], a['elevations'], a['distances'], a['biases'])
        attributes['imnormal'] = None
        return attributes

    def render_recon(self, gt_data, no_mask=False, contour=0, **attributes):
        """render(**attributes) and recon_data(rendered, gt_data, no_mask, contour) in ONE pass over the pixels: the loss terms
        are reduced while the image is shaded and its gradient is formed inside the backward kernels (no loss launches, no dL/drgba
        round trip) -- the path bench.py's `value` times, reachable from the class API.  Returns (loss, rgbs, attributes); ``rgbs``
        carries no gradient here (use render + recon_data if the image feeds anything else that is differentiated).
        contour > 0 (recon_data's contour term, networks.py:379-388; trainer.py:441 passes opt.lambda_contour): folded in as well when the
        image's height and width are multiples of 4 (then the term's two nearest-neighbour resamplings stay inside a screen tile); other
        sizes raise -- call render(...) and recon_data(..., contour=...) for those.  (The reference also prints the term's value there.)"""
        contour = float(contour)
        if contour < 0:
            contour = 0.0                                        # networks.py:379 `if contour>0`
        if contour > 0 and (self.render_height % 4 or self.image_size % 4):
            raise ValueError("render_recon folds the contour term in only for image sizes that are multiples of 4 (got %dx%d); call render(...) and "
                             "recon_data(..., contour=%r)" % (self.render_height, self.image_size, contour))
        a = attributes
        rgba, fn, imn, face_idx, loss = self._render_node(bool(no_mask), gt_data, a['vertices'], a['textures'], a['lights'],
                                                          a['bg'] if no_mask else None, a['azimuths'], a['elevations'], a['distances'], a['biases'],
                                                          contour)
        self._set_outputs(attributes, fn, imn, face_idx)
        return loss, rgba.permute(0, 3, 1, 2), attributes

    # ---- networks.py:364-390 -------------------------------------------------------------------------------------
    def recon_data(self, pred_data, gt_data, no_mask=False, contour=0):
        N.require_device(pred_data, gt_data)
        # (pred_data the untouched image of one of this process's renders: its backward is routed through that render's node -- defer_recon_fusion)
        return N.torch_ext().recon_data(N.fn_addr("mm_recon_query_workspace"), N.fn_addr("mm_recon_data_forward"), N.fn_addr("mm_recon_data_backward"),
                                        pred_data, gt_data, float(self.image_weight), float(contour), N.fn_addr("mm_recon_data_totals"),
                                        bool(self.defer_recon_fusion))

    # ---- networks.py:326-362: seven means in one HIP launch per direction (att_loss.py / csrc/mm_attloss.hip); the chamfer
    # variant of the shape term is a HIP nearest-neighbour search + a differentiable gather ----------
    def recon_att(self, pred_att, target_att, L1=False, chamfer=False, azim=1):
        l = att_loss.attribute_losses(pred_att, target_att, L1)
        loss_cam = azim * l[att_loss.AZIM] + l[att_loss.ELEV] + l[att_loss.DIST]
        if chamfer:
            from .chamfer import chamfer_distance
            loss_shape, _ = chamfer_distance(pred_att['vertices'], target_att['vertices'])
        else:
            loss_shape = l[att_loss.SHAPE]
        return loss_cam, loss_shape, l[att_loss.TEXTURE], 0.1 * l[att_loss.LIGHT], l[att_loss.BIAS]

    # ---- trainer.py:455-494: the disentangle regularisation, seven means in one HIP launch per direction (disentangle.py /
    # csrc/mm_disentangle.hip); with chamfer the two shape terms are composed on the host over the chamfer operator (:469,483) ----
    def recon_disentangle(self, Ae, Ae_fliplr, Ae_jitter, dis1, dis2, azim=1, chamfer=False):
        """``lossR_dis``: dis1 * (l_text + l_shape_flip) + dis2 * ((azim * l_azim + l_elev + l_dist + l_bias) + l_shape_jitter), with
        ``Ae_fliplr = netE(fliplr(Xa))`` and ``Ae_jitter = netE(RandomErasing(p=1)(Xa))`` (``disentangle.disentangle_inputs`` makes both
        batches).  A weight that is not positive drops its half, whose set may then be None; gradients go to all three sets."""
        from . import disentangle as D
        Af = Ae_fliplr if dis1 > 0 else None
        Aj = Ae_jitter if dis2 > 0 else None
        if (dis1 > 0 and Af is None) or (dis2 > 0 and Aj is None):
            raise ValueError("recon_disentangle: dis1 > 0 needs Ae_fliplr and dis2 > 0 needs Ae_jitter")
        lossR_dis = 0.0
        if Af is None and Aj is None:
            return lossR_dis
        l = D.disentangle_terms(Ae, Af, Aj)
        if chamfer:
            from .chamfer import chamfer_distance
        if Af is not None:
            if chamfer:
                Na = Ae['vertices'] * torch.tensor([-1.0, 1.0, 1.0], dtype=Ae['vertices'].dtype, device=Ae['vertices'].device)     # flip x
                l_shape, _ = chamfer_distance(Af['vertices'], Na)
            else:
                l_shape = l[D.SHAPE_FLIP]
            lossR_dis = lossR_dis + dis1 * (l[D.TEXT] + l_shape)
        if Aj is not None:
            if chamfer:
                l_shape, _ = chamfer_distance(Aj['vertices'], Ae['vertices'])
            else:
                l_shape = l[D.SHAPE_JITTER]
            l_cam = azim * l[D.AZIM] + l[D.ELEV] + l[D.DIST] + l[D.BIAS]
            lossR_dis = lossR_dis + dis2 * (l_cam + l_shape)
        return lossR_dis

    # ---- mesh regularisers (networks.py:392-491): HIP kernels, one launch per direction (mesh_reg.py / csrc/mm_reg.hip) ----
    def _reg_tables(self, device):
        key = ("reg", str(device))
        tab = self._static_cache.get(key)
        if tab is None:
            tab = mesh_reg.build_tables(self, device)
            self._static_cache[key] = tab
        return tab

    def _reg(self, terms, vertices=None, delta=None, fn=None, temp=2.0, eps=0.001):
        return mesh_reg.MeshRegFn.apply(self, terms, temp, eps, vertices, delta, fn)

    def recon_flip(self, att, L1):                               # networks.py:392-410
        if L1:
            # the reference multiplies (B,V,3) by (B,V) here and raises (networks.py:409); pinned in tests/golden/losses.npz
            raise RuntimeError("The size of tensor a (3) must match the size of tensor b (%d) at non-singleton dimension 2" % self.num_vertices)
        return self._reg(mesh_reg.mask(mesh_reg.FLIP), delta=att['delta_vertices'])[mesh_reg.FLIP]

    def calc_reg_loss(self, att):                                # networks.py:412-451
        l = self._reg(mesh_reg.mask(mesh_reg.LAPLACIAN, mesh_reg.FLAT), delta=att['delta_vertices'], fn=att['face_normals'])
        return self.lambda_lpl * l[mesh_reg.LAPLACIAN] + self.lambda_flat * l[mesh_reg.FLAT]

    def calc_reg_edge(self, pred):                               # networks.py:453-461
        return self._reg(mesh_reg.mask(mesh_reg.EDGE), vertices=pred)[mesh_reg.EDGE]

    def calc_reg_depth(self, pred):                              # networks.py:463-466
        return self._reg(mesh_reg.mask(mesh_reg.DEPTH), vertices=pred)[mesh_reg.DEPTH]

    def calc_reg_depthR(self, pred, temp=2, eps=0.001):          # networks.py:468-475
        return self._reg(mesh_reg.mask(mesh_reg.DEPTHR), vertices=pred, temp=temp, eps=eps)[mesh_reg.DEPTHR]

    def calc_reg_depthC(self, pred, eps=0.001):                  # networks.py:477-485
        return self._reg(mesh_reg.mask(mesh_reg.DEPTHC), vertices=pred, eps=eps)[mesh_reg.DEPTHC]

    def calc_reg_deform(self, pred):                             # networks.py:487-491
        return self._reg(mesh_reg.mask(mesh_reg.DEFORM), delta=pred)[mesh_reg.DEFORM]

    def regularization(self, Ae, Ai, Aire, opt):
        """trainer.py:54-74 ``regularization(diffRender, Ae, Ai, Aire, opt)`` with every enabled mesh term of an attribute set in
        ONE launch (plus one for its backward) instead of one call per term: returns (lossR_reg, lossR_flip, lossR_IC)."""
        M = mesh_reg
        terms = [M.LAPLACIAN, M.FLAT, M.FLIP]
        for lam, t in ((opt.lambda_edge, M.EDGE), (opt.lambda_depth, M.DEPTH), (opt.lambda_depthR, M.DEPTHR),
                       (opt.lambda_depthC, M.DEPTHC), (opt.lambda_deform, M.DEFORM)):
            if lam > 0:
                terms.append(t)
        if opt.flipL1:
            self.recon_flip(Ae, True)                            # raises, like the reference
        le, li = [self._reg(M.mask(*terms), vertices=A['vertices'], delta=A['delta_vertices'], fn=A['face_normals'],
                            temp=opt.temp) for A in (Ae, Ai)]
        lr = self._reg(M.mask(M.FLIP), delta=Aire['delta_vertices'])
        lossR_reg = opt.lambda_reg * (self.lambda_lpl * (le[M.LAPLACIAN] + li[M.LAPLACIAN]) + self.lambda_flat * (le[M.FLAT] + li[M.FLAT])) / 2.0
        lossR_flip = opt.lambda_flipz * (le[M.FLIP] + li[M.FLIP] + lr[M.FLIP]) / 3.0
        for lam, t in ((opt.lambda_edge, M.EDGE), (opt.lambda_depth, M.DEPTH), (opt.lambda_depthR, M.DEPTHR),
                       (opt.lambda_depthC, M.DEPTHC), (opt.lambda_deform, M.DEFORM)):
            if lam > 0:
                lossR_reg = lossR_reg + lam * (le[t] + li[t]) / 2.0
        parts = self.recon_att(Aire, deep_copy(Ai, detach=True), L1=opt.L1, chamfer=opt.chamfer, azim=opt.azim)
        lossR_IC = opt.lambda_ic * (parts[0] + parts[1] + parts[2] + parts[3] + parts[4])
        return lossR_reg, lossR_flip, lossR_IC


def deep_copy(att, index=None, detach=False):
    """networks.py:146-161 (device follows the attributes instead of the hard-coded 'cuda')."""
    if index is None:
        index = torch.arange(att['distances'].shape[0], device=att['distances'].device)
    copy_att = {}
    for key, value in att.items():
        if key in ('azimuths', 'bg', 'biases', 'elevations', 'distances', 'vertices', 'delta_vertices', 'textures', 'lights'):
            if value is None:
                copy_att[key] = None
            elif detach:
                copy_att[key] = value[index].clone().detach()
            else:
                copy_att[key] = value[index].clone()
    return copy_att
