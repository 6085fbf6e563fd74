// mm_torch_ext.cpp -- the autograd nodes of the class API (DiffRender.render / render_views / render_indexed / render_geometry / recon_data /
// render_recon).
//
// The C ABI of libmm_render.so stays the boundary; this file is PLUMBING above it, compiled with the host compiler only (no device
// code, no HIP headers): one C++ call per autograd node allocates the outputs with ATen, fills the descriptor and enqueues the
// library's launches on torch's current stream -- no Python in any backward (0.12 ms of GPU time per step at B=48, 128x128 leaves
// no room for ~40 Python / ctypes statements per node).  Function addresses of the library come from the ctypes handle, so there is
// no link-time coupling and no second copy of the library.  diff_render.py has no other host path: _native.torch_ext() builds this
// module if it is missing or stale, and raises if it cannot.
#include <torch/extension.h>
#include <torch/csrc/autograd/custom_function.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>      // device guard + current stream of a ROCm build of torch (host headers only)
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/mm_render.h"

namespace {

// ---- DEFERRED FUSION (MMRenderDesc.fused_totals, ABI 6) ---------------------------------------------------------------------------------------
// The un-modified trainer calls `pred, att = render(...)` and later `recon_data(pred, gt)` (trainer.py:276,441).  When that `pred` is the untouched
// image of a render of this process, the loss VALUE is formed by mm_recon_data_forward as always, but its BACKWARD is routed into the render node:
// the render node hands out, next to the image, a one-element `token`; recon_data consumes (token, pred.detach(), gt) instead of (pred, gt); its
// backward returns dL/dloss as the token's gradient and launches nothing; the render node's backward, seeing a token gradient, runs
// mm_render_backward with fused_gt / fused_totals: no dL/drgba tensor, no recon_data backward launch, no read of it by the pixel pass -- and the
// bits mm_recon_data_backward + mm_render_backward would have produced (csrc/mm_pixel_bwd.hip: kDeferred).  Gradients that reach the image from
// its OTHER consumers arrive as grad_rgba as before and are added.
// What a render leaves for a later recon_data to find (keyed by the image's storage address), and what recon_data leaves for the render's backward:
struct Mailbox {
    const void* rgba_ptr = nullptr;
    const void* node = nullptr;             // the render's autograd node (identity of `pred`'s producer)
    uint32_t version = 0;                   // the image's version counter when render returned it
    int64_t B = 0, H = 0, W = 0;
    bool has_token = false;                 // the node declared a fifth output (the token's slot: output_nr 4).  The token TENSOR is not kept here: it would
                                            // close a reference cycle node -> context -> mailbox -> token -> grad_fn -> node that nothing ever frees;
                                            // recon_data makes a fresh tensor and hangs it on the node's output 4 (deferred_token below)
    bool claimed = false;                   // a recon_data has taken this render (a second one runs un-deferred)
    at::Tensor gt, recon_ws;                // recon_data's dense target and its workspace (the totals live in it)
    const float* totals = nullptr;
    double image_weight = 0.0;
};
std::mutex g_mail_mutex;
std::unordered_map<const void*, std::weak_ptr<Mailbox>> g_mail;      // image storage address -> its render's mailbox (weak: dies with the node)

// a 0-byte CPU tensor whose storage context owns a shared_ptr<Mailbox>: the form in which an AutogradContext can hold it (saved_data takes IValues)
void mailbox_deleter(void* ctx) { delete static_cast<std::shared_ptr<Mailbox>*>(ctx); }
at::Tensor mailbox_holder(const std::shared_ptr<Mailbox>& mb) {
    auto* ctx = new std::shared_ptr<Mailbox>(mb);
    c10::DataPtr dp(nullptr, ctx, &mailbox_deleter, c10::Device(c10::kCPU));
    c10::Storage st(c10::Storage::use_byte_size_t(), 0, std::move(dp), nullptr, false);
    return at::empty({0}, at::TensorOptions().dtype(at::kByte)).set_(st, 0, {0}, {1});
}
std::shared_ptr<Mailbox> mailbox_of(const at::Tensor& holder) {
    if (!holder.defined()) return nullptr;
    const c10::DataPtr& dp = holder.storage().data_ptr();
    if (dp.get_deleter() != &mailbox_deleter || !dp.get_context()) return nullptr;
    return *static_cast<std::shared_ptr<Mailbox>*>(dp.get_context());
}

typedef int (*render_fwd_t)(const MMRenderDesc*, void*);
typedef int (*render_bwd_t)(const MMRenderDesc*, const MMRenderGrads*, void*);
typedef int (*recon_t)(const MMReconDesc*, void*);
typedef size_t (*recon_ws_t)(const MMReconDesc*);
typedef int (*render_status_t)(const MMRenderDesc*, void*, int32_t*);
typedef int (*views_fwd_t)(const MMRenderViewsDesc*, void*);
typedef int (*views_bwd_t)(const MMRenderViewsDesc*, const MMRenderGrads*, void*);
typedef int (*indexed_fwd_t)(const MMRenderIndexedDesc*, void*);
typedef int (*indexed_bwd_t)(const MMRenderIndexedDesc*, const MMRenderGrads*, void*);

const float* fptr(const at::Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }
float* mptr(const at::Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }

at::Tensor dense_f32(const at::Tensor& t, const c10::Device& dev, const char* what) {
    TORCH_CHECK(t.is_cuda(), "the MI355X render path needs tensors in device memory (got a ", t.device(), " tensor for ", what, "); there is no CPU fallback");
    if (t.scalar_type() == at::kFloat && t.device() == dev && t.is_contiguous()) return t.detach();
    return t.detach().to(dev, at::kFloat).contiguous();
}

void check(int rc, const char* what) { TORCH_CHECK(rc == MM_OK, what, " failed with status ", rc); }

// The stream a node's work is enqueued on is torch's CURRENT stream of the tensors' device at the time of the call, forward and backward
// alike (the autograd engine re-establishes the forward's stream around a node's backward; a caller driving autograd.grad under another
// stream context gets that one): never a raw handle remembered from the forward, which may be stale by then.  The guard makes the tensors'
// device current for the allocations and the launches.
typedef c10::hip::HIPGuardMasqueradingAsCUDA DeviceGuard;
void* current_stream(const c10::Device& dev) { return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream(); }

MMRenderDesc proto_desc(const std::string& proto) {
    TORCH_CHECK(proto.size() == sizeof(MMRenderDesc), "descriptor prototype of ", proto.size(), " bytes, expected ", sizeof(MMRenderDesc));
    MMRenderDesc d;
    std::memcpy(&d, proto.data(), sizeof d);
    return d;
}

template <class Desc> void bind_workspace(Desc& d, const at::Tensor& ws) { d.workspace = ws.data_ptr(); d.workspace_bytes = (size_t)ws.numel(); }

// ---- what the render nodes share: inputs, outputs, descriptors, gradients, record check, camera shapes -----------------------------------------
using torch::autograd::AutogradContext;
using torch::autograd::tensor_list;

// The dense float32 inputs of a render on one device: vertices, textures, lights and bg per SAMPLE, the cameras per IMAGE and flat
// ((images) / biases (images,2)).  Textures, lights and bg stay undefined where the call has none (geometry only; bg without no_mask).
struct DenseInputs {
    at::Tensor vertices, textures, lights, bg, azimuths, elevations, distances, biases;
    tensor_list list() const { return {vertices, textures, lights, bg, azimuths, elevations, distances, biases}; }
};

// What a render node saves for its backward, by position: DenseInputs::list(), then the forward products the backward re-reads, the workspace
// (alive until the node dies) and, in RenderNode alone, the fused loss's dense target.  The image is not saved: the caller may overwrite it.
enum Saved { S_VERTICES, S_TEXTURES, S_LIGHTS, S_BG, S_AZIMUTHS, S_ELEVATIONS, S_DISTANCES, S_BIASES, S_FACE_IDX, S_FACE_NORMALS, S_WORKSPACE, S_GT };

DenseInputs saved_inputs(const tensor_list& sv) {
    return {sv[S_VERTICES], sv[S_TEXTURES], sv[S_LIGHTS], sv[S_BG], sv[S_AZIMUTHS], sv[S_ELEVATIONS], sv[S_DISTANCES], sv[S_BIASES]};
}

// The caller's tensors as DenseInputs, every shape checked against the prototype `d` of `images` images.  The per-sample tensors carry their own
// row counts: `samples` each in RENDER (and render_geometry: images = samples) and VIEWS (images = samples x views), any count >= 1 in INDEXED.
// VIEWS and INDEXED take the cameras in any shape of `images` values (biases: pairs) and name the counts in their messages.
enum Caller { RENDER, VIEWS, INDEXED };
DenseInputs dense_inputs(const c10::Device& dev, const MMRenderDesc& d, Caller who, int64_t samples, int64_t images, const at::Tensor& vertices,
                         const at::Tensor& textures, const at::Tensor& lights, const c10::optional<at::Tensor>& bg, const at::Tensor& azimuths,
                         const at::Tensor& elevations, const at::Tensor& distances, const at::Tensor& biases) {
    const bool geometry = d.geometry_only == 1;                  // (no textures, lights or bg)
    DenseInputs in;
    in.vertices = dense_f32(vertices, dev, "vertices");
    if (!geometry) { in.textures = dense_f32(textures, dev, "textures"); in.lights = dense_f32(lights, dev, "lights"); }
    // (which error comes first when two inputs are bad: INDEXED has always converted bg before the cameras, the other callers after them)
    auto dense_bg = [&] { if (bg.has_value() && bg->defined()) in.bg = dense_f32(*bg, dev, "bg"); };
    if (who == INDEXED) dense_bg();
    in.azimuths = dense_f32(azimuths, dev, "azimuths").reshape({-1}); in.elevations = dense_f32(elevations, dev, "elevations").reshape({-1});
    in.distances = dense_f32(distances, dev, "distances").reshape({-1}); in.biases = dense_f32(biases, dev, "biases");
    if (who != RENDER) in.biases = in.biases.reshape({-1, 2});
    if (who != INDEXED) dense_bg();
    const at::Tensor &v = in.vertices, &t = in.textures, &l = in.lights, &b = in.biases;
    auto rows_ok = [&](const at::Tensor& x) { return who == INDEXED ? x.size(0) >= 1 : x.size(0) == samples; };
    const bool vertices_ok = v.dim() == 3 && rows_ok(v) && v.size(1) == d.V && v.size(2) == 3;
    const bool textures_ok = geometry || (t.dim() == 4 && rows_ok(t) && t.size(1) == 3 && t.size(2) == d.Ht && t.size(3) == d.Wt);
    const bool lights_ok = geometry || (l.dim() == 2 && rows_ok(l) && l.size(1) == 9);
    const bool bg_ok = !d.no_mask || (in.bg.defined() && in.bg.dim() == 4 && rows_ok(in.bg) && in.bg.size(1) == 3 && in.bg.size(2) == d.H && in.bg.size(3) == d.W);
    const bool cameras_ok = in.elevations.size(0) == images && in.distances.size(0) == images && b.dim() == 2 && b.size(0) == images && b.size(1) == 2;
    if (who != RENDER) {
        const std::string n = who == INDEXED ? "R" : std::to_string(samples);      // how the messages name a tensor's rows
        TORCH_CHECK(in.azimuths.size(0) == images && cameras_ok, who == INDEXED ? "render_indexed: the cameras must hold M = " : "render_views: the cameras must hold B*N = ",
                    images, " values each (biases ", who == INDEXED ? "M" : "B*N", " pairs)");
        TORCH_CHECK(vertices_ok, "vertices must be (", n, ",", d.V, ",3), got ", v.sizes());
        TORCH_CHECK(textures_ok, "textures must be (", n, ",3,", d.Ht, ",", d.Wt, "), got ", t.sizes());
        TORCH_CHECK(lights_ok, "lights must be (", n, ",9), got ", l.sizes());
        TORCH_CHECK(bg_ok, "bg must be (", n, ",3,", d.H, ",", d.W, ")");
    } else {
        TORCH_CHECK(in.azimuths.size(0) == images, "batch size ", in.azimuths.size(0), " does not match the descriptor (", d.B, ")");
        TORCH_CHECK(vertices_ok, "vertices must be (B,", d.V, ",3), got ", v.sizes());
        TORCH_CHECK(textures_ok, "textures must be (B,3,Ht,Wt), got ", t.sizes());
        TORCH_CHECK(lights_ok && cameras_ok, geometry ? "" : "lights (B,9), ", "biases (B,2), elevations/distances (B) expected");
        TORCH_CHECK(bg_ok, "bg must be (B,3,", d.H, ",", d.W, ")");
    }
    return in;
}

void bind_inputs(MMRenderDesc& d, const DenseInputs& in) {
    d.vertices = fptr(in.vertices); d.textures = fptr(in.textures); d.lights = fptr(in.lights); d.bg = d.no_mask ? fptr(in.bg) : nullptr;
    d.azimuths = fptr(in.azimuths); d.elevations = fptr(in.elevations); d.distances = fptr(in.distances); d.biases = fptr(in.biases);
}

// The gradients of the dense inputs (textures and lights only where the call has them, bg only under no_mask) and the MMRenderGrads that points
// at them and at the two upstream gradients (either may be undefined: NULL).
struct RenderGrads {
    at::Tensor vertices, textures, lights, bg, azimuths, elevations, distances, biases;
    MMRenderGrads abi{};
    RenderGrads(const DenseInputs& in, bool no_mask, const at::Tensor& grad_rgba, const at::Tensor& grad_face_normals) {
        vertices = at::empty_like(in.vertices);
        if (in.textures.defined()) { textures = at::empty_like(in.textures); lights = at::empty_like(in.lights); }
        if (no_mask) bg = at::empty_like(in.bg);
        azimuths = at::empty_like(in.azimuths); elevations = at::empty_like(in.elevations); distances = at::empty_like(in.distances);
        biases = at::empty_like(in.biases);
        abi.grad_rgba = fptr(grad_rgba); abi.grad_face_normals = fptr(grad_face_normals);
        abi.grad_vertices = mptr(vertices); abi.grad_textures = mptr(textures); abi.grad_lights = mptr(lights); abi.grad_bg = mptr(bg);
        abi.grad_azimuths = mptr(azimuths); abi.grad_elevations = mptr(elevations); abi.grad_distances = mptr(distances); abi.grad_biases = mptr(biases);
    }
};

// The four outputs of an image-producing node for the leading shape `lead` ({B}, {B,N} or {M}), bound into the forward's descriptor.
struct Outputs {
    at::Tensor rgba, fn, face_idx, imn;
    Outputs(MMRenderDesc& d, std::vector<int64_t> lead, const at::TensorOptions& opts, bool want_imnormal) {
        auto shape = [&lead](std::initializer_list<int64_t> tail) { std::vector<int64_t> s = lead; s.insert(s.end(), tail); return s; };
        rgba = at::empty(shape({d.H, d.W, 4}), opts); fn = at::empty(shape({d.F, 3}), opts);
        face_idx = at::empty(shape({d.H, d.W}), opts.dtype(at::kInt));
        imn = want_imnormal ? at::empty(shape({d.H, d.W, 3}), opts) : at::empty({0}, opts);
        d.rgba = mptr(rgba); d.face_idx = face_idx.data_ptr<int32_t>(); d.face_normals = mptr(fn); d.imnormal = want_imnormal ? mptr(imn) : nullptr;
    }
    // saves enum Saved up to the workspace, then `more`; an output nobody used arrives as an undefined gradient, not as a zero-filled tensor (three
    // allocations + fill launches per step when only the image feeds the loss)
    tensor_list save(AutogradContext* ctx, const DenseInputs& in, const at::Tensor& ws, const tensor_list& more = {}) const {
        tensor_list saved = in.list();
        saved.insert(saved.end(), {face_idx, fn, ws});
        saved.insert(saved.end(), more.begin(), more.end());
        ctx->save_for_backward(saved);
        ctx->mark_non_differentiable({face_idx, imn});
        ctx->set_materialize_grads(false);
        return {rgba, fn, imn, face_idx};
    }
};

// A backward's descriptor, rebuilt from the context's prototype and the saved list (the image is not read back, nor saved: the backward re-forms the
// prediction per pixel), and its two upstream gradients, dense: the normals' may be absent (NULL); the image's is zeros where nothing reached
// the image and `zero_image` asks for them.
struct Backward {
    MMRenderDesc d;
    at::Tensor grgba, gfn;
    Backward(AutogradContext* ctx, const tensor_list& sv, const DenseInputs& in, const tensor_list& g, bool zero_image) : d(proto_desc(ctx->saved_data["proto"].toStringRef())) {
        bind_inputs(d, in); bind_workspace(d, sv[S_WORKSPACE]);
        d.face_idx = sv[S_FACE_IDX].data_ptr<int32_t>(); d.face_normals = mptr(sv[S_FACE_NORMALS]);
        d.rgba = nullptr; d.imnormal = nullptr;
        if (g[0].defined()) grgba = g[0].to(at::kFloat).contiguous();
        else if (zero_image) { auto shape = sv[S_FACE_IDX].sizes().vec(); shape.push_back(4); grgba = at::zeros(shape, in.vertices.options()); }
        if (g[1].defined()) gfn = g[1].to(at::kFloat).contiguous();
    }
};

// a backward's return value, one entry per forward argument: `lead` non-tensors, the gradients of the eight inputs, `trail` more non-tensors
tensor_list input_grads(size_t lead, const RenderGrads& gr, size_t trail) {
    tensor_list out(lead, at::Tensor());
    out.insert(out.end(), {gr.vertices, gr.textures, gr.lights, gr.bg, gr.azimuths, gr.elevations, gr.distances, gr.biases});
    out.resize(out.size() + trail);
    return out;
}

// DiffRender.check_texture_records (f_status: mm_render_status, or 0): a diagnostic after a backward -- it synchronises the stream.  `d` is the
// backward's descriptor of `images` images; their render workspace starts `offset` bytes into the node's (render_views: behind the staging head).
void check_texture_records(int64_t f_status, MMRenderDesc d, void* stream, int64_t images, size_t offset, const char* call, const char* whose) {
    if (!f_status) return;
    d.workspace = (char*)d.workspace + offset; d.workspace_bytes -= offset;
    std::vector<int32_t> dropped((size_t)images);
    const int st = ((render_status_t)f_status)(&d, stream, dropped.data());
    std::string list;
    bool any = false;
    for (int32_t n : dropped) { list += (list.empty() ? "" : ", ") + std::to_string(n); any = any || n != 0; }
    TORCH_CHECK(!(st == MM_ERR_WORKSPACE && any), call, ": the texture-record pool overflowed (records dropped per image: [", list,
                "]); the texture gradients of those ", whose, " are NaN. Raise DiffRender.extra_texture_records_per_pixel.");
    check(st, "mm_render_status");
}

// the cameras may arrive as (B), (B,1), (B,N), ...: the kernels see them flat, the gradients go back in the caller's shapes (advisor r05)
void save_camera_shapes(AutogradContext* ctx, const at::Tensor& azimuths, const at::Tensor& elevations, const at::Tensor& distances, const at::Tensor& biases) {
    ctx->saved_data["shape_a"] = azimuths.sizes().vec(); ctx->saved_data["shape_e"] = elevations.sizes().vec();
    ctx->saved_data["shape_d"] = distances.sizes().vec(); ctx->saved_data["shape_b"] = biases.sizes().vec();
}
void restore_camera_shapes(AutogradContext* ctx, RenderGrads& g) {
    auto restore = [ctx](at::Tensor& t, const char* key) {          // (a camera that arrived flat keeps its tensor: no view is made)
        const at::DimVector shape = ctx->saved_data[key].toDimVector();
        if (!t.sizes().equals(shape)) t = t.reshape(shape);
    };
    restore(g.azimuths, "shape_a"); restore(g.elevations, "shape_e"); restore(g.distances, "shape_d"); restore(g.biases, "shape_b");
}

// ---- recon_data --------------------------------------------------------------------------------------------------------------------------------
// the descriptor of a (B,4,H,W) prediction with its own strides against a dense target; the workspace is bound if there is one yet
MMReconDesc recon_desc(const at::Tensor& pred, const at::Tensor& gt, const at::Tensor& ws, double image_weight, double contour) {
    MMReconDesc d{};
    d.B = (int32_t)pred.size(0); d.H = (int32_t)pred.size(2); d.W = (int32_t)pred.size(3);
    d.pred = fptr(pred); d.gt = fptr(gt);
    for (int i = 0; i < 4; ++i) d.pred_strides[i] = pred.stride(i);
    d.image_weight = (float)image_weight; d.contour = (float)contour;
    if (ws.defined()) bind_workspace(d, ws);
    return d;
}

// loss, dense prediction, dense target, workspace
std::vector<at::Tensor> recon_forward(int64_t f_ws, int64_t f_fwd, at::Tensor pred, at::Tensor gt, double image_weight, double contour, void* stream) {
    TORCH_CHECK(pred.is_cuda() && gt.is_cuda(), "the MI355X render path needs tensors in device memory; there is no CPU fallback");
    const c10::Device dev = pred.device();
    pred = pred.detach().to(at::kFloat);
    if (!pred.is_non_overlapping_and_dense()) pred = pred.contiguous();
    gt = gt.detach().to(dev, at::kFloat).contiguous();
    TORCH_CHECK(pred.dim() == 4 && pred.size(1) == 4 && gt.sizes() == pred.sizes(), "recon_data expects (B,4,H,W) prediction and target, got ", pred.sizes(), " / ", gt.sizes());
    at::Tensor loss = at::empty({}, pred.options());
    MMReconDesc d = recon_desc(pred, gt, at::Tensor(), image_weight, contour);
    d.loss = mptr(loss);
    at::Tensor ws = at::empty({(int64_t)((recon_ws_t)f_ws)(&d)}, pred.options().dtype(at::kByte));
    bind_workspace(d, ws);
    check(((recon_t)f_fwd)(&d, stream), "mm_recon_data_forward");
    return {loss, pred, gt, ws};
}

// the live mailbox of the render whose image starts at `rgba_ptr`, if any
std::shared_ptr<Mailbox> find_mailbox(const void* rgba_ptr) {
    std::lock_guard<std::mutex> lock(g_mail_mutex);
    auto it = g_mail.find(rgba_ptr);
    return it != g_mail.end() ? it->second.lock() : nullptr;
}

// ---- the autograd nodes themselves, in C++: no Python (and no GIL hand-over to the autograd thread) in the backward -----------------------
// DiffRender.render / render_recon.  Outputs: rgba (B,H,W,4), face_normals (B,F,3), imnormal (B,H,W,3 or empty), face_idx (B,H,W) int32, then the
// loss (gt given: the fused loss) or the deferred-fusion token (defer).  The backward returns the gradients of vertices, textures, lights, bg
// (undefined unless no_mask), azimuths, elevations, distances, biases.
class RenderNode : public torch::autograd::Function<RenderNode> {
 public:
    static tensor_list forward(AutogradContext* ctx, int64_t f_fwd, int64_t f_loss, int64_t f_bwd, int64_t f_status, std::string proto, int64_t ws_bytes,
                               at::Tensor vertices, at::Tensor textures, at::Tensor lights, c10::optional<at::Tensor> bg, at::Tensor azimuths,
                               at::Tensor elevations, at::Tensor distances, at::Tensor biases, c10::optional<at::Tensor> gt, bool want_imnormal,
                               double image_weight, bool defer) {
        TORCH_CHECK(azimuths.is_cuda(), "the MI355X render path needs tensors in device memory; there is no CPU fallback");
        const c10::Device dev = azimuths.device();
        const DeviceGuard guard(dev);
        save_camera_shapes(ctx, azimuths, elevations, distances, biases);
        at::Tensor ws = at::empty({ws_bytes}, azimuths.options().dtype(at::kByte));   // (the caching allocator is the workspace pool)
        MMRenderDesc d = proto_desc(proto);
        const int64_t B = d.B, H = d.H, W = d.W;
        const DenseInputs in = dense_inputs(dev, d, RENDER, B, B, vertices, textures, lights, bg, azimuths, elevations, distances, biases);
        auto opts = in.vertices.options();
        const Outputs out(d, {B}, opts, want_imnormal);
        at::Tensor loss, gtt;
        bind_inputs(d, in); bind_workspace(d, ws);
        const bool fused = gt.has_value() && gt->defined();
        if (fused) {
            gtt = dense_f32(*gt, dev, "gt_data");
            TORCH_CHECK(gtt.dim() == 4 && gtt.size(0) == B && gtt.size(1) == 4 && gtt.size(2) == H && gtt.size(3) == W, "gt_data must be (B,4,", H, ",", W, "), got ", gtt.sizes());
            loss = at::empty({}, opts);
            d.fused_gt = fptr(gtt); d.fused_image_weight = (float)image_weight; d.fused_loss = mptr(loss);
        }
        void* stream = current_stream(dev);
        check(((render_fwd_t)f_fwd)(&d, stream), "mm_render_forward");
        if (fused) check(((render_fwd_t)f_loss)(&d, stream), "mm_render_fused_loss");
        ctx->saved_data["f_bwd"] = f_bwd; ctx->saved_data["f_status"] = f_status; ctx->saved_data["proto"] = proto;
        ctx->saved_data["image_weight"] = image_weight;
        tensor_list ret = out.save(ctx, in, ws, {gtt});          // (enum Saved)
        if (fused) ctx->mark_non_differentiable({out.rgba});
        if (fused) ret.push_back(loss);
        else if (defer) {
            // deferred fusion: a fifth output whose only job is to carry dL/dloss of a later recon_data(image, gt) back into THIS node (never read, never
            // written: no launch), and the mailbox that recon_data finds through the image's address
            auto mb = std::make_shared<Mailbox>();
            mb->rgba_ptr = out.rgba.data_ptr(); mb->B = B; mb->H = H; mb->W = W;
            mb->has_token = true;
            ctx->saved_data["mb"] = mailbox_holder(mb);
            { std::lock_guard<std::mutex> lock(g_mail_mutex);
              if (g_mail.size() > 256) for (auto it = g_mail.begin(); it != g_mail.end();) it = it->second.expired() ? g_mail.erase(it) : std::next(it);
              g_mail[mb->rgba_ptr] = mb; }
            ret.push_back(at::empty({1}, opts));                 // (declares output 4 and its metadata; dropped by render_node)
        }
        return ret;
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list g) {
        const auto sv = ctx->get_saved_variables();
        const DenseInputs in = saved_inputs(sv);
        const c10::Device dev = in.azimuths.device();
        const DeviceGuard guard(dev);
        const bool token_grad = g.size() > 4 && g[4].defined();  // of output 4: the fused loss, or the token a recon_data routed its dL/dloss through
        // deferred fusion: a recon_data consumed this render's image and its loss takes part in what is differentiated (the token has a gradient)
        std::shared_ptr<Mailbox> mb;
        if (!sv[S_GT].defined() && token_grad && ctx->saved_data.count("mb")) mb = mailbox_of(ctx->saved_data["mb"].toTensor());
        const bool deferred = mb && mb->gt.defined() && mb->totals != nullptr;
        TORCH_CHECK(deferred || sv[S_GT].defined() || !token_grad, "a recon_data token carries a gradient but its render has no recon_data on record");
        // deferred: target, weight and totals come from the recon_data that consumed the image; fused: from this node's own forward
        const at::Tensor& gt = deferred ? mb->gt : sv[S_GT];
        const double image_weight = deferred ? mb->image_weight : ctx->saved_data["image_weight"].toDouble();
        const bool fused = gt.defined();
        Backward b(ctx, sv, in, g, !fused);
        MMRenderDesc& d = b.d;
        at::Tensor gloss;
        if (fused) {
            // An undefined gradient of the loss output means the loss took no part in what is being differentiated (materialize_grads is off):
            // its gradient is ZERO, never one -- e.g. reg.backward() through attributes['face_normals'] only.
            gloss = token_grad ? g[4].to(at::kFloat).reshape({}).contiguous() : at::zeros({}, in.vertices.options().dtype(at::kFloat));
            d.fused_gt = fptr(gt); d.fused_image_weight = (float)image_weight; d.fused_grad_loss = fptr(gloss);
            if (deferred) { d.fused_totals = mb->totals; d.fused_contour = 0.f; }    // (b.grgba: the image's other consumers, added by the kernel)
            else b.grgba = at::Tensor();                         // the fused loss alone drives the image
        }
        RenderGrads gr(in, d.no_mask, b.grgba, b.gfn);
        void* stream = current_stream(dev);
        check(((render_bwd_t)ctx->saved_data["f_bwd"].toInt())(&d, &gr.abi, stream), "mm_render_backward");
        check_texture_records(ctx->saved_data["f_status"].toInt(), d, stream, d.B, 0, "mm_render_backward", "images");
        restore_camera_shapes(ctx, gr);
        return input_grads(6, gr, 4);
    }
};

// recon_data on the untouched image of a render that handed out a token (deferred fusion, top of this file): the forward is mm_recon_data_forward on
// the image as always (same launches, same value); the backward launches NOTHING -- dL/dloss travels to the render node as the token's gradient.
class ReconDeferredNode : public torch::autograd::Function<ReconDeferredNode> {
 public:
    static at::Tensor forward(AutogradContext* ctx, at::Tensor token, at::Tensor holder, int64_t f_ws, int64_t f_fwd, int64_t f_tot, at::Tensor pred,
                              at::Tensor gt, double image_weight) {
        const DeviceGuard guard(pred.device());
        (void)token;
        auto out = recon_forward(f_ws, f_fwd, pred, gt, image_weight, 0.0, current_stream(pred.device()));
        auto mb = mailbox_of(holder);
        TORCH_CHECK(mb, "deferred recon_data without its render's mailbox");
        const MMReconDesc d = recon_desc(out[1], out[2], out[3], image_weight, 0.0);
        typedef const float* (*totals_t)(const MMReconDesc*);
        mb->totals = ((totals_t)f_tot)(&d);
        TORCH_CHECK(mb->totals != nullptr, "mm_recon_data_totals failed");
        mb->gt = out[2]; mb->recon_ws = out[3]; mb->image_weight = image_weight;     // alive as long as the render node is
        ctx->set_materialize_grads(false);
        return out[0];
    }
    static tensor_list backward(AutogradContext* ctx, tensor_list g) {
        (void)ctx;
        at::Tensor gt;                                           // the token's gradient = dL/dloss (one float on the device; a view where the caller's is one)
        if (g[0].defined()) gt = g[0].to(at::kFloat).reshape({1});
        return {gt, at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
    }
};

class ReconNode : public torch::autograd::Function<ReconNode> {
 public:
    static at::Tensor forward(AutogradContext* ctx, int64_t f_ws, int64_t f_fwd, int64_t f_bwd, at::Tensor pred, at::Tensor gt, double image_weight,
                              double contour) {
        TORCH_CHECK(pred.is_cuda(), "the MI355X render path needs tensors in device memory; there is no CPU fallback");
        const DeviceGuard guard(pred.device());
        auto out = recon_forward(f_ws, f_fwd, pred, gt, image_weight, contour, current_stream(pred.device()));
        ctx->saved_data["f_bwd"] = f_bwd; ctx->saved_data["image_weight"] = image_weight; ctx->saved_data["contour"] = contour;
        ctx->save_for_backward({out[1], out[2], out[3]});
        return out[0];
    }
    static tensor_list backward(AutogradContext* ctx, tensor_list g) {
        const auto sv = ctx->get_saved_variables();               // dense prediction, dense target, workspace
        const at::Tensor& pred = sv[0];
        const DeviceGuard guard(pred.device());
        at::Tensor g_loss = g[0].to(pred.device(), at::kFloat).contiguous();
        at::Tensor grad = at::empty_strided(pred.sizes(), pred.strides(), pred.options());
        MMReconDesc d = recon_desc(pred, sv[1], sv[2], ctx->saved_data["image_weight"].toDouble(), ctx->saved_data["contour"].toDouble());
        d.grad_loss = fptr(g_loss); d.grad_pred = mptr(grad);
        check(((recon_t)ctx->saved_data["f_bwd"].toInt())(&d, current_stream(pred.device())), "mm_recon_data_backward");
        return {at::Tensor(), at::Tensor(), at::Tensor(), grad, at::Tensor(), at::Tensor(), at::Tensor()};
    }
};

// DiffRender.render_geometry (MMRenderDesc.geometry_only: the vertex stage alone, for the render whose image trainer.py:367 discards):
// face_normals (B,F,3) with a backward to vertices and the four camera inputs.  The prototype carries geometry_only = 1.
class GeometryNode : public torch::autograd::Function<GeometryNode> {
 public:
    static at::Tensor forward(AutogradContext* ctx, int64_t f_fwd, int64_t f_bwd, std::string proto, int64_t ws_bytes, at::Tensor vertices,
                              at::Tensor azimuths, at::Tensor elevations, at::Tensor distances, at::Tensor biases) {
        TORCH_CHECK(azimuths.is_cuda(), "the MI355X render path needs tensors in device memory; there is no CPU fallback");
        const c10::Device dev = azimuths.device();
        const DeviceGuard guard(dev);
        MMRenderDesc d = proto_desc(proto);
        TORCH_CHECK(d.geometry_only == 1, "GeometryNode needs a geometry-only descriptor prototype");
        save_camera_shapes(ctx, azimuths, elevations, distances, biases);
        const DenseInputs in = dense_inputs(dev, d, RENDER, d.B, d.B, vertices, at::Tensor(), at::Tensor(), c10::nullopt, azimuths, elevations, distances, biases);
        at::Tensor ws = at::empty({ws_bytes}, azimuths.options().dtype(at::kByte));
        at::Tensor fn = at::empty({(int64_t)d.B, (int64_t)d.F, 3}, in.vertices.options());
        bind_inputs(d, in); bind_workspace(d, ws);
        d.face_normals = mptr(fn);
        check(((render_fwd_t)f_fwd)(&d, current_stream(dev)), "mm_render_forward (geometry only)");
        ctx->saved_data["f_bwd"] = f_bwd; ctx->saved_data["proto"] = proto;
        tensor_list saved = in.list();
        saved.insert(saved.end(), {at::Tensor(), at::Tensor(), ws});   // (enum Saved; the backward reads neither face_idx nor the normals)
        ctx->save_for_backward(saved);
        ctx->set_materialize_grads(false);
        return fn;
    }
    static tensor_list backward(AutogradContext* ctx, tensor_list g) {
        tensor_list none(9);
        if (!g[0].defined()) return none;                        // face_normals took no part in what is differentiated
        const auto sv = ctx->get_saved_variables();
        const DenseInputs in = saved_inputs(sv);
        const c10::Device dev = in.azimuths.device();
        const DeviceGuard guard(dev);
        MMRenderDesc d = proto_desc(ctx->saved_data["proto"].toStringRef());
        at::Tensor gfn = g[0].to(at::kFloat).contiguous();
        bind_inputs(d, in); bind_workspace(d, sv[S_WORKSPACE]);
        d.face_normals = mptr(gfn);                              // (a valid pointer for the argument check; the backward does not read the normals)
        RenderGrads gr(in, false, at::Tensor(), gfn);
        check(((render_bwd_t)ctx->saved_data["f_bwd"].toInt())(&d, &gr.abi, current_stream(dev)), "mm_render_backward (geometry only)");
        restore_camera_shapes(ctx, gr);
        none[4] = gr.vertices; none[5] = gr.azimuths; none[6] = gr.elevations; none[7] = gr.distances; none[8] = gr.biases;
        return none;
    }
};

// DiffRender.render_views (MMRenderViewsDesc: B samples x N views in one pass over B*N images; the per-sample tensors are read from their single
// copy, their gradients are the view-order sums).  The prototype is the MMRenderDesc of the B*N images; the cameras arrive as (B,N) / (B,N,2)
// (an expanded (B,) input gets its gradient through autograd's own expand); outputs are (B,N,...).  No fused loss, no deferred fusion.
class RenderViewsNode : public torch::autograd::Function<RenderViewsNode> {
 public:
    static tensor_list forward(AutogradContext* ctx, int64_t f_fwd, int64_t f_bwd, int64_t f_status, std::string proto, int64_t views, int64_t ws_bytes,
                               int64_t staging_bytes, at::Tensor vertices, at::Tensor textures, at::Tensor lights, c10::optional<at::Tensor> bg, at::Tensor azimuths,
                               at::Tensor elevations, at::Tensor distances, at::Tensor biases, bool want_imnormal) {
        TORCH_CHECK(azimuths.is_cuda(), "the MI355X render path needs tensors in device memory; there is no CPU fallback");
        const c10::Device dev = azimuths.device();
        const DeviceGuard guard(dev);
        MMRenderDesc d = proto_desc(proto);                          // (of the B*N images)
        const int64_t N = views, BN = d.B;
        TORCH_CHECK(N >= 1 && BN % N == 0, "render_views: ", BN, " images are not a multiple of ", N, " views");
        const int64_t B = BN / N;
        save_camera_shapes(ctx, azimuths, elevations, distances, biases);
        const DenseInputs in = dense_inputs(dev, d, VIEWS, B, BN, vertices, textures, lights, bg, azimuths, elevations, distances, biases);
        auto opts = in.vertices.options();
        const Outputs out(d, {B, N}, opts, want_imnormal);
        at::Tensor ws = at::empty({ws_bytes}, opts.dtype(at::kByte));
        bind_inputs(d, in); bind_workspace(d, ws);
        const MMRenderViewsDesc vd{d, (int32_t)views};
        check(((views_fwd_t)f_fwd)(&vd, current_stream(dev)), "mm_render_views_forward");
        ctx->saved_data["f_bwd"] = f_bwd; ctx->saved_data["f_status"] = f_status; ctx->saved_data["proto"] = proto; ctx->saved_data["views"] = views;
        ctx->saved_data["staging_bytes"] = staging_bytes;            // the head of the workspace (the per-image gradients' staging): mm_render_status skips it
        return out.save(ctx, in, ws);                                // (enum Saved: the UN-replicated inputs)
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list g) {
        const auto sv = ctx->get_saved_variables();
        const DenseInputs in = saved_inputs(sv);
        const c10::Device dev = in.azimuths.device();
        const DeviceGuard guard(dev);
        const Backward b(ctx, sv, in, g, true);
        const MMRenderDesc& d = b.d;
        RenderGrads gr(in, d.no_mask, b.grgba, b.gfn);
        void* stream = current_stream(dev);
        const MMRenderViewsDesc vd{d, (int32_t)ctx->saved_data["views"].toInt()};
        check(((views_bwd_t)ctx->saved_data["f_bwd"].toInt())(&vd, &gr.abi, stream), "mm_render_views_backward");
        // per IMAGE, as in render: the render workspace of the B*N images lies behind the staging head of the multi-view workspace
        check_texture_records(ctx->saved_data["f_status"].toInt(), d, stream, d.B, (size_t)ctx->saved_data["staging_bytes"].toInt(),
                              "mm_render_views_backward", "samples");
        restore_camera_shapes(ctx, gr);
        return input_grads(7, gr, 1);
    }
};

// DiffRender.render_indexed (MMRenderIndexedDesc: M images in one pass, each reading the row of vertices / textures / lights / bg its index names;
// the gradients of those four are the sums over each row's images in ascending image order and have the inputs' own shapes).  The prototype is the
// MMRenderDesc of the M images; an index is an (M) int32 tensor on the device or undefined (the identity).  backward: an input requires grad -- only
// then does the workspace (ws_bytes, sized by the caller for that flag) hold the staging areas.  head_bytes: the workspace's head (plan + staging),
// which mm_render_status skips; status_word: the address the plan adds its count of out-of-range index entries to.
struct IndexTensors { at::Tensor t[4]; };
void bind_indexed(MMRenderIndexedDesc& vd, const MMRenderDesc& d, const DenseInputs& in, const IndexTensors& ix, bool backward, int64_t status_word) {
    vd.render = d;
    vd.rows[0] = (int32_t)in.vertices.size(0); vd.rows[1] = (int32_t)in.textures.size(0); vd.rows[2] = (int32_t)in.lights.size(0);
    vd.rows[3] = in.bg.defined() ? (int32_t)in.bg.size(0) : d.B;
    for (int k = 0; k < 4; ++k) vd.index[k] = ix.t[k].defined() ? ix.t[k].data_ptr<int32_t>() : nullptr;
    vd.backward = backward ? 1 : 0;
    vd.status_flag = (int32_t*)status_word;
}

class RenderIndexedNode : public torch::autograd::Function<RenderIndexedNode> {
 public:
    static tensor_list forward(AutogradContext* ctx, int64_t f_fwd, int64_t f_bwd, int64_t f_status, std::string proto, int64_t ws_bytes, int64_t head_bytes,
                               int64_t status_word, bool backward, at::Tensor vertices, at::Tensor textures, at::Tensor lights, c10::optional<at::Tensor> bg,
                               at::Tensor azimuths, at::Tensor elevations, at::Tensor distances, at::Tensor biases, c10::optional<at::Tensor> idx_vertices,
                               c10::optional<at::Tensor> idx_textures, c10::optional<at::Tensor> idx_lights, c10::optional<at::Tensor> idx_bg,
                               bool want_imnormal) {
        TORCH_CHECK(azimuths.is_cuda(), "the MI355X render path needs tensors in device memory; there is no CPU fallback");
        const c10::Device dev = azimuths.device();
        const DeviceGuard guard(dev);
        MMRenderDesc d = proto_desc(proto);                          // (of the M images)
        const int64_t M = d.B;
        save_camera_shapes(ctx, azimuths, elevations, distances, biases);
        const DenseInputs in = dense_inputs(dev, d, INDEXED, 0, M, vertices, textures, lights, bg, azimuths, elevations, distances, biases);
        IndexTensors ix;
        const c10::optional<at::Tensor>* given[4] = {&idx_vertices, &idx_textures, &idx_lights, &idx_bg};
        for (int k = 0; k < 4; ++k) {
            if (!given[k]->has_value() || !(*given[k])->defined() || (k == 3 && !d.no_mask)) continue;
            const at::Tensor& t = **given[k];
            TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous() && t.dim() == 1 && t.size(0) == M,
                        "render_indexed: an index must be a contiguous (", M, ") int32 tensor in device memory");
            ix.t[k] = t;
        }
        auto opts = in.vertices.options();
        const Outputs out(d, {M}, opts, want_imnormal);
        at::Tensor ws = at::empty({ws_bytes}, opts.dtype(at::kByte));
        bind_inputs(d, in); bind_workspace(d, ws);
        MMRenderIndexedDesc vd{};
        bind_indexed(vd, d, in, ix, backward, status_word);
        check(((indexed_fwd_t)f_fwd)(&vd, current_stream(dev)), "mm_render_indexed_forward");
        ctx->saved_data["f_bwd"] = f_bwd; ctx->saved_data["f_status"] = f_status; ctx->saved_data["proto"] = proto;
        ctx->saved_data["head_bytes"] = head_bytes; ctx->saved_data["status_word"] = status_word; ctx->saved_data["backward"] = backward;
        return out.save(ctx, in, ws, {at::Tensor(), ix.t[0], ix.t[1], ix.t[2], ix.t[3]});     // (enum Saved: the UN-gathered inputs; then the four indices)
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list g) {
        const auto sv = ctx->get_saved_variables();
        const DenseInputs in = saved_inputs(sv);
        const c10::Device dev = in.azimuths.device();
        const DeviceGuard guard(dev);
        TORCH_CHECK(ctx->saved_data["backward"].toBool(), "render_indexed: the forward ran without an input that requires grad and kept no staging");
        const Backward b(ctx, sv, in, g, true);
        const MMRenderDesc& d = b.d;
        RenderGrads gr(in, d.no_mask, b.grgba, b.gfn);               // (the indexed inputs' gradients in the inputs' own shapes)
        void* stream = current_stream(dev);
        IndexTensors ix;
        for (int k = 0; k < 4; ++k) ix.t[k] = sv[S_GT + 1 + k];
        MMRenderIndexedDesc vd{};
        bind_indexed(vd, d, in, ix, true, ctx->saved_data["status_word"].toInt());
        check(((indexed_bwd_t)ctx->saved_data["f_bwd"].toInt())(&vd, &gr.abi, stream), "mm_render_indexed_backward");
        // per IMAGE, as in render: the render workspace of the M images lies behind the head of the indexed workspace
        check_texture_records(ctx->saved_data["f_status"].toInt(), d, stream, d.B, (size_t)ctx->saved_data["head_bytes"].toInt(),
                              "mm_render_indexed_backward", "images");
        restore_camera_shapes(ctx, gr);
        return input_grads(8, gr, 5);
    }
};

tensor_list render_indexed_node(int64_t f_fwd, int64_t f_bwd, int64_t f_status, std::string proto, int64_t ws_bytes, int64_t head_bytes, int64_t status_word,
                                bool backward, at::Tensor vertices, at::Tensor textures, at::Tensor lights, c10::optional<at::Tensor> bg, at::Tensor azimuths,
                                at::Tensor elevations, at::Tensor distances, at::Tensor biases, c10::optional<at::Tensor> idx_vertices,
                                c10::optional<at::Tensor> idx_textures, c10::optional<at::Tensor> idx_lights, c10::optional<at::Tensor> idx_bg, bool want_imnormal) {
    return RenderIndexedNode::apply(f_fwd, f_bwd, f_status, proto, ws_bytes, head_bytes, status_word, backward, vertices, textures, lights, bg, azimuths, elevations,
                                    distances, biases, idx_vertices, idx_textures, idx_lights, idx_bg, want_imnormal);
}

tensor_list render_views_node(int64_t f_fwd, int64_t f_bwd, int64_t f_status, std::string proto, int64_t views, int64_t ws_bytes, int64_t staging_bytes,
                              at::Tensor vertices, at::Tensor textures, at::Tensor lights, c10::optional<at::Tensor> bg, at::Tensor azimuths,
                              at::Tensor elevations, at::Tensor distances, at::Tensor biases, bool want_imnormal) {
    return RenderViewsNode::apply(f_fwd, f_bwd, f_status, proto, views, ws_bytes, staging_bytes, vertices, textures, lights, bg, azimuths, elevations, distances, biases,
                                  want_imnormal);
}

at::Tensor geometry_node(int64_t f_fwd, int64_t f_bwd, std::string proto, int64_t ws_bytes, at::Tensor vertices, at::Tensor azimuths, at::Tensor elevations,
                         at::Tensor distances, at::Tensor biases) {
    return GeometryNode::apply(f_fwd, f_bwd, proto, ws_bytes, vertices, azimuths, elevations, distances, biases);
}

// defer: hand out the token a later recon_data(image, gt) can route its backward through (deferred fusion; the returned list is still
// {rgba, face_normals, imnormal, face_idx}: the token lives in the mailbox)
tensor_list render_node(int64_t f_fwd, int64_t f_loss, int64_t f_bwd, int64_t f_status, std::string proto, int64_t ws_bytes, at::Tensor vertices,
                        at::Tensor textures, at::Tensor lights, c10::optional<at::Tensor> bg, at::Tensor azimuths, at::Tensor elevations,
                        at::Tensor distances, at::Tensor biases, c10::optional<at::Tensor> gt, bool want_imnormal, double image_weight, bool defer) {
    const bool fused = gt.has_value() && gt->defined();
    defer = defer && !fused && at::GradMode::is_enabled();
    tensor_list out = RenderNode::apply(f_fwd, f_loss, f_bwd, f_status, proto, ws_bytes, vertices, textures, lights, bg, azimuths, elevations, distances,
                                        biases, gt, want_imnormal, image_weight, defer);
    if (defer && out.size() > 4) {
        auto mb = find_mailbox(out[0].data_ptr());
        if (mb && out[0].grad_fn() && out[4].grad_fn().get() == out[0].grad_fn().get() && out[4].output_nr() == 4) {
            mb->node = out[0].grad_fn().get(); mb->version = out[0]._version();
        } else if (mb) mb->claimed = true;                       // nothing requires grad: no backward will ever run, nothing to defer
        out.pop_back();
    }
    return out;
}

// The render whose image `pred` is, if recon_data may route its backward through it: pred is the (B,4,H,W) permute view of (or the NHWC image itself,
// seen as (B,4,H,W)) output 0 of a render node that handed out a token, float32, never modified in place since, not yet taken by another recon_data.
std::shared_ptr<Mailbox> deferrable_render(const at::Tensor& pred) {
    if (!pred.defined() || !pred.is_cuda() || pred.scalar_type() != at::kFloat || pred.dim() != 4 || !pred.requires_grad() || !at::GradMode::is_enabled()) return nullptr;
    auto mb = find_mailbox(pred.data_ptr());
    if (!mb || mb->claimed || !mb->node || !mb->has_token) return nullptr;
    if (pred.size(0) != mb->B || pred.size(1) != 4 || pred.size(2) != mb->H || pred.size(3) != mb->W) return nullptr;
    if (pred.stride(0) != 4 * mb->H * mb->W || pred.stride(1) != 1 || pred.stride(2) != 4 * mb->W || pred.stride(3) != 4) return nullptr;
    if (pred._version() != mb->version) return nullptr;         // written in place since the render returned it
    const auto fn = pred.grad_fn();
    if (!fn) return nullptr;
    // `pred` must BE the render's image: one permute away from output 0 of the node (what DiffRender.render returns)
    if (fn->num_inputs() < 1 || fn->next_edges().size() != 1) return nullptr;
    const auto& e = fn->next_edge(0);
    if (e.function.get() != mb->node || e.input_nr != 0 || fn->name().find("Permute") == std::string::npos) return nullptr;
    return mb;
}

// a one-element tensor that IS output 4 of `pred`'s render node as far as autograd is concerned: whatever gradient reaches it arrives in that node's
// backward as g[4].  (`pred` has passed deferrable_render: its grad_fn is the permute whose only input edge is the node's output 0.)
at::Tensor deferred_token(const at::Tensor& pred) {
    at::Tensor tok = at::empty({1}, pred.options());
    torch::autograd::impl::set_gradient_edge(tok, torch::autograd::Edge(pred.grad_fn()->next_edge(0).function, 4));
    return tok;
}

at::Tensor recon_node(int64_t f_ws, int64_t f_fwd, int64_t f_bwd, at::Tensor pred, at::Tensor gt, double image_weight, double contour, int64_t f_tot,
                      bool allow_defer) {
    if (allow_defer && f_tot != 0 && !(contour > 0.0)) {
        if (auto mb = deferrable_render(pred)) {
            mb->claimed = true;
            // (find the holder again through the node's context is not possible from here: a second holder of the same mailbox travels as an argument)
            return ReconDeferredNode::apply(deferred_token(pred), mailbox_holder(mb), f_ws, f_fwd, f_tot, pred.detach(), gt, image_weight);
        }
    }
    return ReconNode::apply(f_ws, f_fwd, f_bwd, pred, gt, image_weight, contour);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("render", &render_node);
    m.def("recon_data", &recon_node);
    m.def("render_geometry", &geometry_node);
    m.def("render_views", &render_views_node);
    m.def("render_indexed", &render_indexed_node);
    m.def("desc_bytes", []() { return (int64_t)sizeof(MMRenderDesc); });
    m.def("deferrable", [](at::Tensor pred) { return deferrable_render(pred) != nullptr; });   // tests / diagnostics: would recon_data(pred, .) defer?
}
