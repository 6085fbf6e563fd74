"""FID around the network on the MI355X (csrc/mm_fid.hip) against the restatements and references of tests/test_fid_host.py.

``inception_input`` is held to ``inception_input_host`` with ``torch.equal``: both round every fp32 step as written.  ``FidStatistics.finalize``
is held to the longdouble reference by the host file's two derived bounds, and with ``==`` to the rational result of the exact integer
case -- a wrong fragment map of the f64 MFMA puts results into other rows and fails it.  ``fid_score`` equals its public pieces composed by
hand."""
import importlib

import numpy as np
import pytest
import torch

from test_fid_host import (INPUT_SHAPES, STATS_SHAPES, exact_expected, exact_features, features, input_frames, stats_violations)

pytestmark = pytest.mark.gpu

FID = importlib.import_module("3d-magic-mirror_amd.fid")
DEV = torch.device("cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def finalized(x, batch=None, **kw):
    st = FID.FidStatistics(x.shape[1], **kw)
    for i in range(0, x.shape[0], batch or x.shape[0]):
        st.update(dev(x[i:i + (batch or x.shape[0])]))
    return st.finalize()


# ---- inception_input ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", INPUT_SHAPES)
def test_input_equals_the_restatement(H, W):
    f = input_frames(H, W, n=3)
    for size, normalize in ((299, True), (299, False), (1, True), (None, True), (None, False)):
        got = FID.inception_input(dev(f), size, normalize)
        want = FID.inception_input_host(f, size, normalize)
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == want.shape
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (size, normalize)


def test_input_alignments_strides_and_out():
    H, W = 37, 21
    f = input_frames(H, W, n=2)
    want = torch.from_numpy(FID.inception_input_host(f, 299, True))
    flat = torch.zeros(f.size + 16, dtype=torch.uint8, device=DEV)
    for off in (1, 2, 3):                                                 # frames that start at odd byte offsets
        flat[off:off + f.size] = dev(f).reshape(-1)
        assert torch.equal(FID.inception_input(flat[off:off + f.size].view(2, H, W, 3)).cpu(), want)
    wide = torch.zeros((2, H, W + 5, 3), dtype=torch.uint8, device=DEV)   # a view that is not contiguous
    wide[:, :, 2:2 + W] = dev(f)
    view = wide[:, :, 2:2 + W]
    assert not view.is_contiguous() and torch.equal(FID.inception_input(view).cpu(), want)
    assert torch.equal(FID.inception_input(dev(f[0])).cpu(), want[:1])    # one (H,W,3) frame is n = 1
    out = torch.full((2, 3, 299, 299), float("nan"), device=DEV)
    assert FID.inception_input(dev(f), out=out) is out and torch.equal(out.cpu(), want)
    store = torch.full((2 * 3 * 5 * 7 + 1,), float("nan"), device=DEV)     # an out= that is not 16-byte aligned: the one-by-one stores
    out = store[1:].view(2, 3, 5, 7)
    assert FID.inception_input(dev(f[:, :5, :7]), size=None, out=out) is out
    assert torch.equal(out.cpu(), torch.from_numpy(FID.inception_input_host(f[:, :5, :7], None, True))) and bool(torch.isnan(store[0]))
    with pytest.raises(ValueError):
        FID.inception_input(dev(f), out=torch.empty((2, 3, 298, 299), device=DEV))


# ---- FidStatistics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", STATS_SHAPES + [(8, 2048)])
def test_statistics_within_the_bounds(N, D):
    x = features(N, D)
    mu, sigma = finalized(x)
    assert mu.dtype == sigma.dtype == torch.float64 and tuple(mu.shape) == (D,) and tuple(sigma.shape) == (D, D) and mu.is_cuda
    assert stats_violations(mu.cpu().numpy(), sigma.cpu().numpy(), x) == (0, 0)
    assert torch.equal(sigma, sigma.T)
    mu2, sigma2 = finalized(x)                                            # a second run: the same bits
    assert torch.equal(mu, mu2) and torch.equal(sigma, sigma2)


def test_statistics_exact_case():
    x = exact_features()
    mu, sigma = finalized(x)
    want_mu, want_sigma = exact_expected(x)
    assert np.all(mu.cpu().numpy() == want_mu)
    assert np.all(sigma.cpu().numpy() == want_sigma)


def test_statistics_batches_capacity_and_widening():
    x = features(300, 33)
    mu, sigma = finalized(x)
    for batch in (1, 7, 64):
        m, s = finalized(x, batch=batch)
        assert torch.equal(m, mu) and torch.equal(s, sigma), batch
    m, s = finalized(x, batch=64, capacity=300)                           # preallocated against grown (1024 rows at first)
    assert torch.equal(m, mu) and torch.equal(s, sigma)
    m, s = finalized(features(1030, 5), batch=7)                          # grows past the first 1024 rows
    assert stats_violations(m.cpu().numpy(), s.cpu().numpy(), features(1030, 5)) == (0, 0)
    h = x.astype(np.float16)                                              # float16 and bfloat16 are widened exactly; (b,D,1,1) is (b,D)
    st = FID.FidStatistics(33).update(dev(h).reshape(300, 33, 1, 1))
    m, s = finalized(h.astype(np.float32))
    assert all(torch.equal(a, b) for a, b in zip(st.finalize(), (m, s)))
    b16 = dev(x).bfloat16()
    st = FID.FidStatistics(33).update(b16)
    assert all(torch.equal(a, b) for a, b in zip(st.finalize(), finalized(b16.float().cpu().numpy())))
    with pytest.raises(ValueError, match="at least two"):
        FID.FidStatistics(33).update(dev(x[:1])).finalize()


# ---- fid_score ----------------------------------------------------------------------------------------------------------------------
def test_fid_score_is_its_pieces():
    jpeg = importlib.import_module("3d-magic-mirror_amd.jpeg")
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 16, 7, stride=8), torch.nn.ReLU(), torch.nn.AdaptiveAvgPool2d(1)).to(DEV)
    rng = np.random.default_rng(5)
    a = dev(rng.integers(0, 256, (20, 32, 16, 3), dtype=np.uint8))
    b = dev((rng.integers(0, 256, (20, 32, 16, 3)) // 2 + 64).astype(np.uint8))

    def by_hand(frames):
        st = FID.FidStatistics(16)
        with torch.no_grad():
            for i in range(0, 20, 8):                                     # the tail batch of 4 is included
                st.update(model(FID.inception_input(frames[i:i + 8])))
        assert st.n == 20
        return st

    sa, sb = by_hand(a), by_hand(b)
    want = FID.frechet_distance(*sa.finalize(), *sb.finalize())
    got = FID.fid_score(a, b, model, batch_size=8)
    assert isinstance(got, float) and got == want and got > 0
    assert FID.fid_score(sa, b, model, batch_size=8) == want == FID.fid_score(a, sb, model, batch_size=8) == FID.fid_score(sa, sb, model)
    one = FID.FidStatistics.from_frames(a, model, batch_size=8)
    assert one.n == 20 and all(torch.equal(p, q) for p, q in zip(one.finalize(), sa.finalize()))
    saved = FID.fid_score(a, b, model, batch_size=8, as_saved=True, quality=90)
    assert saved == FID.fid_score(jpeg.jpeg_roundtrip(a, 90), jpeg.jpeg_roundtrip(b, 90), model, batch_size=8) != want
