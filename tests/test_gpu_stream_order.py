"""Every operator on a delayed side stream against its own default-stream bits (tests/stream_order.py has the protocol and the table).

What a default-stream suite cannot see: a piece of an operator that does not run on the stream it was given (a torch helper op, a memset,
a backward that reads the stream differently from its forward), and a resident table that one stream uploads and another reads.  The
canary runs first and shows that the set-up can see such a thing at all: a side stream here is not implicitly ordered with stream 0, and
the delay is long enough to expose it.  No graph capture (step.py's capture has its own tests), no new processes."""
import importlib
import os

import numpy as np
import pytest
import torch

import stream_order as SO

pytestmark = pytest.mark.gpu

N = importlib.import_module("3d-magic-mirror_amd._native")


def test_00_canary_a_side_stream_is_not_ordered_with_the_default_stream():
    """A plain copy behind a delay into a pre-filled buffer, read on the default stream without waiting: the read sees the pre-fill
    (stream_order.side_streams: every test below runs on streams that have shown this)."""
    side = SO.side_streams(1)[0]
    assert SO._independent(side), "the stream the cases run on is ordered with the default stream: they would pass whatever the operators do"
    cal = SO.MEASURED["calibration"]
    print("delay calibration: %d %s took %.2f ms -> %.0f per ms; streams tried: %d"
          % (cal["probe_units"], cal["kind"], cal["probe_ms"], cal["units_per_ms"], SO.MEASURED["streams_tried"]))


def test_01_the_protocol_fails_an_operator_that_launches_on_another_stream():
    """export_images called under the default stream from inside the side stream's block: it reads the decoy, and the comparison says so"""
    c = SO.BY_NAME["export_images"]

    def off_stream(x):
        with torch.cuda.stream(torch.cuda.default_stream(x.device)):
            return c.op(x)
    with pytest.raises(AssertionError, match="differs in"):
        SO.run_behind_delay(c.make_inputs, off_stream)
    SO.run_behind_delay(c.make_inputs, c.op)


@pytest.mark.parametrize("name", [c.name for c in SO.CASES])
def test_operator_behind_a_delay_has_its_default_stream_bits(name, monkeypatch):
    c = SO.BY_NAME[name]
    called = SO.record_exports(monkeypatch, sorted(SO.stream_exports()))
    SO.run_behind_delay(c.make_inputs, c.op, syncs=bool(c.syncs), name=name)
    print("%s: enqueued in %.2f ms" % (name, SO.MEASURED["enqueue_ms"].get(name, float("nan"))))
    assert called <= set(c.exports), "exports called through _native.call / fn that the case does not declare: %s" % sorted(called - set(c.exports))
    through_python = set(c.exports) - set(c.by_address)
    assert through_python <= called, "declared exports the case never called: %s" % sorted(through_python - called)


# ---- backward called from outside the stream block ----------------------------------------------------------------------------------
def _backward_outside(ran):
    ran[1].backward()
    return [t.grad for t in ran[2].values() if torch.is_tensor(t) and t.requires_grad]


def test_backward_from_the_default_stream_runs_the_cpp_node_on_its_forwards_stream():
    def forward(att, gt):
        loss, made, a = SO.render_recon_forward(att, gt)
        return [loss.detach()] + made, loss, a
    got = SO.run_behind_delay(SO.render_inputs, forward, name=None, backward=_backward_outside)
    assert len(got) == 4 + len(SO.LEAVES)


def test_backward_from_the_default_stream_runs_the_python_function_on_its_forwards_stream():
    def forward(X, Y):
        per_image, made, a = SO.ssim_forward(X, Y)
        return [per_image.detach()], (per_image * per_image).sum(), a
    got = SO.run_behind_delay(SO.images_inputs((2, 3, 24, 20)), forward, name=None, backward=_backward_outside)
    assert len(got) == 3


# ---- two streams at once -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("export_images", "composite_frames", "jpeg_roundtrip", "inception_input"))
def test_two_side_streams_at_once(name):
    """two calls with different inputs, each on a side stream of its own behind a delay, both enqueued before either is waited for: the
    wrappers allocate their workspaces and tables per call, and each result has its own default-stream bits"""
    c = SO.BY_NAME[name]
    dev = SO.device()
    seeds = (SO.TRUE_SEED, SO.DECOY_SEED)
    inputs = [SO.on_device(c.make_inputs(s), dev) for s in seeds]
    want = [SO.flat(c.op(*a)) for a in inputs]
    torch.cuda.synchronize(dev)
    assert any(not torch.equal(x, y) for x, y in zip(want[0], want[1]))
    streams = SO.side_streams(2)
    got, delaying = [], []
    for s, a in zip(streams, inputs):
        with torch.cuda.stream(s):
            delaying.append(SO.delay(s))
            got.append(SO.flat(c.op(*a)))
    busy = [not e.query() for e in delaying]
    torch.cuda.synchronize(dev)
    assert all(busy), "a delay had ended before both calls were enqueued"
    for g, w in zip(got, want):
        SO.same_bits(g, w, name)


# ---- hand-off of every resident table -------------------------------------------------------------------------------------------------
def _hand_off(first_call, cached, sources, second_call):
    """The first call of a fresh key on a side stream behind the delay; then, before any consumer is launched elsewhere, the cached device
    tensors cloned on the default stream and held to their host sources; only then the second call on the default stream while the side
    stream is busy again.  Returns (first result, second result) as flat lists, after a synchronise."""
    dev = SO.device()
    side = SO.side_streams(1)[0]
    with torch.cuda.stream(side):
        SO.delay(side)
        first = SO.flat(first_call())
    clones = [t.clone() for t in cached()]                               # default stream, at once: a table that is finished on return is whole here
    want = [torch.as_tensor(np.ascontiguousarray(s)) if isinstance(s, np.ndarray) else s for s in sources()]
    clones = [t.cpu() for t in clones]
    assert len(clones) == len(want) and len(want) > 0
    for i, (t, s) in enumerate(zip(clones, want)):
        assert t.dtype == s.dtype and t.shape == s.shape, (i, t.dtype, s.dtype, tuple(t.shape), tuple(s.shape))
        assert torch.equal(t.contiguous().view(torch.uint8), s.contiguous().view(torch.uint8)), \
            "resident table %d was not whole when the call that uploaded it returned: no consumer is launched on it" % i
    # The upload's wait has drained the side stream, so it is made busy again for the second call -- after the host reads above: where
    # the two streams share a hardware queue a blocking read on the default stream would wait for the delay.
    delaying = SO.delay(side)
    second = SO.flat(second_call())
    busy = not delaying.query()
    torch.cuda.synchronize(dev)
    assert busy, "the side stream's delay had ended when the second call returned"
    return first, second


def test_hand_off_fid_tables():
    F = importlib.import_module("3d-magic-mirror_amd.fid")
    dev = SO.device()
    H, W, size = 11, 13, 37                                              # a key no other test uses
    frames = SO.frames_of(5, (2, H, W, 3)).to(dev)
    want = torch.from_numpy(F.inception_input_host(frames.cpu().numpy(), size, True)).to(dev)
    torch.cuda.synchronize(dev)
    F._TABLES.clear()
    key = (H, W, size, frames.device)
    first, second = _hand_off(lambda: F.inception_input(frames, size), lambda: [F._TABLES[key][3]], lambda: [F._TABLES[key][2]],
                              lambda: F.inception_input(frames, size))
    SO.same_bits(first, [want], "first call, side stream")
    SO.same_bits(second, [want], "second call, default stream")


def test_hand_off_jpeg_resident_params():
    J = importlib.import_module("3d-magic-mirror_amd.jpeg")
    dev = SO.device()
    H, W, q = 11, 13, 83
    frames = SO.frames_of(6, (2, H, W, 3)).to(dev)
    J._resident_params.cache_clear()
    want = SO.flat(J.jpeg_roundtrip(frames, q))
    torch.cuda.synchronize(dev)
    J._resident_params.cache_clear()
    first, second = _hand_off(lambda: J.jpeg_roundtrip(frames, q), lambda: [J._resident_params(frames.device, H, W, q, "4:2:0")],
                              lambda: [J.lower_jpeg(H, W, q)["params"]], lambda: J.jpeg_roundtrip(frames, q))
    SO.same_bits(first, want, "first call, side stream")
    SO.same_bits(second, want, "second call, default stream")


def test_hand_off_lpl_tables():
    EF = importlib.import_module("3d-magic-mirror_amd.encoder_features")
    dev = SO.device()
    template, lpl = SO.template_and_lpl()
    x, w, p = SO.on_device(SO.encfeat_inputs("shape")(SO.TRUE_SEED), dev)
    tmpl = SO.template_on_device()
    want = EF.shape_features(x, tmpl, lpl, p)
    torch.cuda.synchronize(dev)
    fresh = lpl.clone()                                                  # a tensor the cache has not seen
    m = fresh.to(torch.float32)
    first, second = _hand_off(lambda: EF.shape_features(x, tmpl, fresh, p), lambda: list(EF.lpl_tables(fresh, x.device)),
                              lambda: list(EF._ell_columns(m)) + list(EF._ell_columns(m.t())), lambda: EF.shape_features(x, tmpl, fresh, p))
    SO.same_bits(first, [want], "first call, side stream")
    SO.same_bits(second, [want], "second call, default stream")


def test_hand_off_diff_render_static_and_mesh_reg_tables():
    pkg = SO.mod()
    MR = SO.mod("mesh_reg")
    dev = SO.device()
    att, gt = SO.on_device(SO.render_inputs(SO.TRUE_SEED), dev)
    sets = SO.on_device(SO.reg_inputs(SO.TRUE_SEED), dev)
    old = SO.renderer(SO.S_RENDER)

    def render(dr):
        with torch.no_grad():
            rgbs, out = dr.render(no_mask=True, **att)
        return [rgbs, out["face_normals"], dr.last_face_idx]

    def reg(dr):
        with torch.no_grad():
            return dr._reg(MR.mask(MR.LAPLACIAN, MR.FLAT, MR.EDGE, MR.FLIP), vertices=sets[0]["vertices"], delta=sets[0]["delta_vertices"],
                           fn=sets[0]["face_normals"])
    want_render, want_reg = SO.flat(render(old)), SO.flat(reg(old))
    torch.cuda.synchronize(dev)
    dr = pkg.DiffRender(os.path.join(SO.TEMPLATES, "sphere.npz"), SO.S_RENDER, emit_imnormal=True)      # a fresh object: nothing of it is resident yet
    st = lambda: dr._static(dev)
    first, second = _hand_off(lambda: render(dr), lambda: [st()[k] for k in ("faces", "face_uvs", "vc_table")],
                              lambda: [dr.faces.to(torch.int32), dr.face_uvs.to(torch.float32).reshape(-1, 3, 2), dr._vc_table.to(torch.int32)],
                              lambda: render(dr))
    SO.same_bits(first, want_render, "render: first call, side stream")
    SO.same_bits(second, want_render, "render: second call, default stream")
    host = {}

    def host_tables():                                                   # build_tables' numpy sources, by running it for the host
        if not host:
            host.update(MR.build_tables(dr, "cpu"))
        return host
    keys = sorted(k for k in host_tables() if k != "E")
    first, second = _hand_off(lambda: reg(dr), lambda: [dr._reg_tables(dev)[k] for k in keys], lambda: [host_tables()[k] for k in keys], lambda: reg(dr))
    SO.same_bits(first, want_reg, "mesh regulariser: first call, side stream")
    SO.same_bits(second, want_reg, "mesh regulariser: second call, default stream")
