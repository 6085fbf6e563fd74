"""The table of tests/stream_order.py without a device: the census of the exports that take a stream, and every case's decoy through
the wrappers' own argument checks.

The census is what keeps the table complete: an export added to ``_native.SIGNATURES`` that returns a status is taken to launch on a
stream unless ``stream_order.EXCLUDED`` excludes it with a reason, and then fails ``test_every_stream_export_has_a_case`` until a case names it."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import stream_order as SO

N = importlib.import_module("3d-magic-mirror_amd._native")
PKG = os.path.dirname(os.path.abspath(N.__file__))

EXCLUDED, NO_DEVICE_INPUTS, stream_exports = SO.EXCLUDED, SO.NO_DEVICE_INPUTS, SO.stream_exports


def test_exclusions_are_exports_without_a_stream_or_a_caller():
    import ctypes
    for name in EXCLUDED:
        assert N.SIGNATURES[name][0] is ctypes.c_int, name
    header = open(os.path.join(os.path.dirname(PKG), "include", "mm_render.h")).read()
    for name in stream_exports():                                 # and every export that is kept does take one, by the header
        assert re.search(r"\b%s\([^;]*mm_stream_t stream" % name, header), name
    for name in set(EXCLUDED) - {"mm_jpeg_encode"}:
        assert not re.search(r"\b%s\([^;]*mm_stream_t" % name, header), name


def test_mm_jpeg_encode_has_no_caller():
    """no module names the export as a string (fn, call, fn_addr) or as an attribute of the library; prose may mention it"""
    for root, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".cpp")) and f != "_native.py":
                assert not re.search(r"""["'.]mm_jpeg_encode\b["'(]""", open(os.path.join(root, f)).read()), f


def test_every_stream_export_has_a_case():
    declared = set().union(*[set(c.exports) for c in SO.CASES])
    want = stream_exports()
    assert declared - want == set(), "cases name exports that take no stream: %s" % sorted(declared - want)
    assert want - declared == set(), "exports that take a stream and have no case in tests/stream_order.py: %s" % sorted(want - declared)


def test_every_host_wait_is_named():
    for c in SO.CASES:
        assert c.syncs is False or (isinstance(c.syncs, str) and len(c.syncs) > 20), c.name
        assert set(c.by_address) <= set(c.exports), c.name


@pytest.mark.parametrize("name", [c.name for c in SO.CASES])
def test_decoy_is_a_legal_input_and_differs(name):
    c = SO.BY_NAME[name]
    true, decoy = c.make_inputs(SO.TRUE_SEED), c.make_inputs(SO.DECOY_SEED)
    assert c.check is not None, "a case without its wrapper's argument checks"
    c.check(*decoy)
    c.check(*true)
    a, b = SO.tensors_of(true), SO.tensors_of(decoy)
    assert len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.stride() == y.stride() for x, y in zip(a, b))
    assert not any(t.is_cuda for t in a + b)
    if name in NO_DEVICE_INPUTS:
        assert not a
        return
    differ = [not torch.equal(x, y) for x, y in zip(a, b) if x.dtype not in (torch.int32, torch.int64)]      # (an index into one row has one legal value)
    assert differ and all(differ), "every input of the decoy differs from the true one"
    again = SO.tensors_of(c.make_inputs(SO.TRUE_SEED))             # and the inputs are a function of the seed alone
    assert all(np.array_equal(x.numpy(), y.numpy(), equal_nan=True) for x, y in zip(a, again))
