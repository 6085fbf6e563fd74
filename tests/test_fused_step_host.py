"""Host-side contract of step mode (MMRenderDesc.step_grads): the binding mirrors the grown descriptor, the workspace query accounts for the
step arrays only when the field is set, and mm_render_step_mode answers from sizes, options and pointers alone -- no GPU needed."""
import ctypes
import importlib

import pytest


@pytest.fixture(scope="module")
def N(pkg):
    return importlib.import_module("3d-magic-mirror_amd._native")


def _desc(N, B=48, H=128, W=128, F=1280, V=642, Ht=256, Wt=128):
    d = N.MMRenderDesc()
    d.B, d.H, d.W, d.V, d.F, d.Ht, d.Wt, d.knum, d.no_mask = B, H, W, V, F, Ht, Wt, 30, 1
    return d


def test_descriptor_ends_with_the_step_field_and_sizes_agree(N):
    L = N.lib()
    assert L.mm_struct_size(0) == ctypes.sizeof(N.MMRenderDesc)
    assert N.MMRenderDesc.step_grads.offset == ctypes.sizeof(N.MMRenderDesc) - ctypes.sizeof(ctypes.c_void_p)
    assert N.MMRenderDesc.step_grads.offset > N.MMRenderDesc.fused_totals.offset


def test_workspace_grows_only_with_the_field_set(N):
    L = N.lib()
    d = _desc(N)
    base = L.mm_query_workspace(ctypes.byref(d))
    g = N.MMRenderGrads()
    d.step_grads = ctypes.addressof(g)
    step = L.mm_query_workspace(ctypes.byref(d))
    blocks, rc_min = (128 // 16) ** 2, 128 * 128 * 9 // 8
    assert step - base == 48 * 4 * blocks * 12 * 4 + 48 * rc_min * 8         # one light row per tile + one run descriptor per minimum record slot
    lay, lay_step = (ctypes.c_size_t * 12)(), (ctypes.c_size_t * 12)()
    d0 = _desc(N)
    assert L.mm_debug_workspace_layout(ctypes.byref(d0), lay) == 0 and L.mm_debug_workspace_layout(ctypes.byref(d), lay_step) == 0
    assert list(lay) == list(lay_step)                                       # nothing in front of the step arrays moves


def test_step_mode_is_taken_only_under_its_conditions(N):
    L = N.lib()
    g = N.MMRenderGrads()
    bg = ctypes.c_float()
    g.grad_bg = ctypes.addressof(bg)
    gt = (ctypes.c_float * 4)()

    def mode(**kw):
        d = _desc(N, **{k: v for k, v in kw.items() if k in ("B", "H", "W", "F")})
        d.step_grads, d.fused_gt = ctypes.addressof(g), ctypes.addressof(gt)
        for k, v in kw.items():
            if k not in ("B", "H", "W", "F"):
                setattr(d, k, v)
        return L.mm_render_step_mode(ctypes.byref(d))

    assert mode() == 1
    assert mode(step_grads=None) == 0 and mode(fused_gt=None) == 0
    assert mode(fused_contour=0.5) == 0 and mode(fused_totals=ctypes.addressof(gt)) == 0 and mode(geometry_only=1) == 0
    assert mode(options=N.OPT_MANY_IN_FLIGHT) == 0 and mode(options=N.OPT_WALK_WAVE) == 0 and mode(options=N.OPT_WALK_QUEUE) == 0
    assert mode(B=384) == 0                                                  # the one-tile-per-workgroup walk of large batches
    assert mode(H=512, W=512, F=13776) == 0                                  # screen bins larger than a tile: the compacting walk
    g2 = N.MMRenderGrads()                                                   # no_mask without a grad_bg to write
    assert mode(step_grads=ctypes.addressof(g2)) == 0 and mode(step_grads=ctypes.addressof(g2), no_mask=0) == 1
