"""FID around the network, on the host (3d-magic-mirror_amd/fid.py): the numpy restatements that tests/test_gpu_fid.py holds the kernels to, held
here to independent references; ``frechet_distance`` against closed forms and a ``scipy.linalg.sqrtm`` composition; validation, the ``.npz``
round trip and the ABI rows.  Nothing here needs a GPU.

Inception inputs: ``inception_input_host`` within 1e-6 of ``F.interpolate`` composed in float64 and then ``2 x - 1`` -- the chain has
fewer than ten fp32 roundings on magnitudes of at most 1, and sixteen roundings of 2^-24 are 9.5e-7.

Statistics: ``fid_statistics_host`` against a ``np.longdouble`` computation, elementwise with ``<=`` (a constant column has bound 0 and error 0):
    |sigma - ref| <= (N + 4) * 2^-53 * (|Xc|^T |Xc|) / (N - 1)        |mu - ref| <= N * 2^-53 * mean|x|
A float64 sum of N + 3 terms (N products, the centring's two roundings folded in, the division) is off by at most that many units of the
sum of magnitudes to first order; plain ``np.cov`` stays within 0.26 and 0.15 of the two."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

FID = importlib.import_module("3d-magic-mirror_amd.fid")
SPLIT, TILE = FID.FID_SPLIT, FID.FID_TILE

INPUT_SHAPES = [(1, 1), (3, 5), (128, 64), (299, 299), (300, 301), (400, 37)]
INPUT_MODES = [(299, True), (299, False), (1, True), (1, False), (None, True), (None, False)]
STATS_SHAPES = [(2, 1), (5, 17), (300, 33), (1030, 48), (3, 16), (4, 15), (SPLIT - 1, 17), (SPLIT, 17), (SPLIT + 1, 17),
                (9, TILE - 1), (9, TILE), (9, TILE + 1)]
FAULTS = ["div_n", "drop_tail", "uncentred", "no_mirror"]
U = 2.0 ** -53


def input_frames(H, W, n=2, seed=0):
    return np.random.default_rng(seed + 1000 * H + W).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def input_reference(frames, size, normalize):
    """the float64 composition: v / 255, F.interpolate, 2 x - 1"""
    x = torch.from_numpy(frames).permute(0, 3, 1, 2).double() / 255.0
    if size is not None:
        x = F.interpolate(x, (size, size), mode="bilinear", align_corners=False)
    return (2.0 * x - 1.0 if normalize else x).numpy()


def features(N, D, seed=0):
    """the issue's inputs: 3 * rng.random as float32"""
    return (3 * np.random.default_rng(seed + 131 * N + D).random((N, D))).astype(np.float32)


def exact_features():
    """N = 64 rows of integers in [-7, 7], D = 33: every centred value (a multiple of 1/64), product and sum is exact in float64"""
    return np.random.default_rng(7).integers(-7, 8, (64, 33)).astype(np.float32)


def exact_expected(x):
    """the rational result of exact_features, divided once by 63: (mu, sigma)"""
    xi = x.astype(np.int64)
    n = xi.shape[0]
    s = xi.sum(0)
    c = n * xi - s                                              # n * (x - mean): integers
    g = c.T @ c                                                 # n^2 * Gram, exact in int64
    return s.astype(np.float64) / n, (g.astype(np.float64) / (n * n)) / (n - 1)


_REF = {}


def stats_reference(x):
    """(mu, sigma, bound_mu, bound_sigma) in np.longdouble; computed once per array"""
    key = (x.shape, hash(x.tobytes()))
    if key not in _REF:
        X = x.astype(np.longdouble)
        n = X.shape[0]
        mu = X.sum(0) / n
        Xc = X - mu
        sigma = (Xc.T @ Xc) / (n - 1)
        b_mu = n * np.longdouble(U) * np.abs(X).sum(0) / n
        b_sigma = (n + 4) * np.longdouble(U) * (np.abs(Xc).T @ np.abs(Xc)) / (n - 1)
        _REF[key] = (mu, sigma, b_mu, b_sigma)
    return _REF[key]


def stats_violations(mu, sigma, x):
    """how many elements of (mu, sigma) miss the two bounds against the longdouble reference"""
    r_mu, r_sigma, b_mu, b_sigma = stats_reference(x)
    bad_mu = np.abs(np.asarray(mu).astype(np.longdouble) - r_mu) > b_mu
    bad_sigma = np.abs(np.asarray(sigma).astype(np.longdouble) - r_sigma) > b_sigma
    return int(bad_mu.sum()), int(bad_sigma.sum())


# ---- Inception inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", INPUT_SHAPES)
def test_input_restatement_is_the_float64_composition(H, W):
    f = input_frames(H, W)
    for size, normalize in INPUT_MODES:
        got = FID.inception_input_host(f, size, normalize)
        S = (H, W) if size is None else (size, size)
        assert got.dtype == np.float32 and got.shape == (2, 3) + S and got.flags.c_contiguous
        err = float(np.abs(got.astype(np.float64) - input_reference(f, size, normalize)).max())
        print("inception_input_host %dx%d size %r normalize %r: max error %.3g" % (H, W, size, normalize, err))
        assert err <= 1e-6


def test_input_at_the_networks_size_is_the_identity():
    f = input_frames(299, 299, n=1)
    t = (np.arange(256, dtype=np.float32) / np.float32(255.0))[f].transpose(0, 3, 1, 2)
    assert np.array_equal(FID.inception_input_host(f, 299, False), t)
    assert np.array_equal(FID.inception_input_host(f, 299, True), np.float32(2) * t - np.float32(1))
    assert np.array_equal(FID.inception_input_host(f, None, True), FID.inception_input_host(f, 299, True))
    assert np.array_equal(FID.inception_input_host(f[0], 299, True), FID.inception_input_host(f, 299, True))      # one frame is n = 1


def test_input_table_stays_inside_its_axes():
    for H, W in INPUT_SHAPES + [(1024, 1024), (1, 1024)]:
        for size in (299, 1, 1024, None):
            Ho, Wo, rows = FID.lower_inception_input(H, W, size)
            assert rows.shape == (Wo + Ho, 4) and rows.dtype == np.int32
            for r, n_in in ((rows[:Wo], W), (rows[Wo:], H)):
                w = np.ascontiguousarray(r[:, 2:]).view(np.float32)
                assert r[:, :2].min() >= 0 and r[:, :2].max() < n_in and np.all(r[:, 0] <= r[:, 1])
                assert np.all(w >= 0) and np.all(np.abs(w.astype(np.float64).sum(1) - 1) <= 2.0 ** -24)


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", STATS_SHAPES)
def test_statistics_restatement_within_the_bounds(N, D):
    x = features(N, D)
    mu, sigma = FID.fid_statistics_host(x)
    assert mu.dtype == sigma.dtype == np.float64 and mu.shape == (D,) and sigma.shape == (D, D)
    assert stats_violations(mu, sigma, x) == (0, 0)
    assert np.array_equal(sigma, sigma.T)
    r_mu, r_sigma, b_mu, b_sigma = stats_reference(x)                     # how far plain numpy is: inside both bounds too
    assert np.all(np.abs(np.cov(x.astype(np.float64), rowvar=False).reshape(D, D) - r_sigma) <= b_sigma)
    assert np.all(np.abs(x.astype(np.float64).mean(0) - r_mu) <= b_mu)


def test_statistics_of_a_constant_column_are_exact():
    x = features(37, 5)
    x[:, 2] = 1.25
    mu, sigma = FID.fid_statistics_host(x)
    assert mu[2] == 1.25 and np.all(sigma[2] == 0) and np.all(sigma[:, 2] == 0)
    assert stats_violations(mu, sigma, x) == (0, 0)


def test_statistics_exact_case():
    x = exact_features()
    mu, sigma = FID.fid_statistics_host(x)
    want_mu, want_sigma = exact_expected(x)
    assert np.all(mu == want_mu) and np.all(sigma == want_sigma)
    assert stats_violations(mu, sigma, x) == (0, 0)


@pytest.mark.parametrize("fault", FAULTS)
def test_the_cases_catch_each_fault(fault):
    """a restatement with one fault misses a bound in at least one of the shapes, and the exact case where the fault can show there"""
    caught = []
    for N, D in STATS_SHAPES:
        if N > 1100:
            continue                                                     # (the long cases add nothing here)
        x = features(N, D)
        if sum(stats_violations(*FID.fid_statistics_host(x, fault=fault), x)) > 0:
            caught.append((N, D))
    assert caught, fault
    if fault == "drop_tail":
        assert all(N % 4 for N, _ in caught) and (5, 17) in caught and (3, 16) in caught
    else:
        assert (300, 33) in caught and (9, TILE + 1) in caught
        x = exact_features()
        mu, sigma = FID.fid_statistics_host(x, fault=fault)
        assert not np.all(sigma == exact_expected(x)[1])


# ---- frechet_distance ---------------------------------------------------------------------------------------------------------------
def sqrtm_distance(mu1, s1, mu2, s2):
    """the reference's route without its branches: scipy.linalg.sqrtm of the product, the real part's trace"""
    import scipy.linalg
    root = scipy.linalg.sqrtm(s1.dot(s2))
    d = mu1 - mu2
    return float(d.dot(d) + np.trace(s1) + np.trace(s2) - 2 * np.trace(np.real(root)))


def orthogonal(D, rng):
    q, r = np.linalg.qr(rng.standard_normal((D, D)))
    return q * np.sign(np.diag(r))


def test_frechet_commuting_covariances():
    rng = np.random.default_rng(1)
    Q = orthogonal(64, rng)
    a, b = rng.uniform(0.1, 10, 64), rng.uniform(0.1, 10, 64)
    mu1, mu2 = rng.standard_normal(64), rng.standard_normal(64)
    s1, s2 = (Q * a) @ Q.T, (Q * b) @ Q.T
    s1, s2 = (s1 + s1.T) / 2, (s2 + s2.T) / 2
    want = float(((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((mu1 - mu2) ** 2).sum())
    got = FID.frechet_distance(mu1, s1, mu2, s2)
    assert isinstance(got, float) and abs(got - want) <= 1e-10 * (a.sum() + b.sum())
    assert got == FID.frechet_distance(*(torch.from_numpy(t) for t in (mu1, s1, mu2, s2)))         # tensors and arrays alike


def test_frechet_two_by_two():
    rng = np.random.default_rng(2)
    for _ in range(20):
        A, B = rng.standard_normal((2, 2)), rng.standard_normal((2, 2))
        s1, s2 = A @ A.T + 0.1 * np.eye(2), B @ B.T + 0.1 * np.eye(2)
        P = s1 @ s2
        tr_root = np.sqrt(np.trace(P) + 2 * np.sqrt(np.linalg.det(P)))
        mu = rng.standard_normal(2)
        want = float(np.trace(s1) + np.trace(s2) - 2 * tr_root)
        assert abs(FID.frechet_distance(mu, s1, mu, s2) - want) <= 1e-10 * (np.trace(s1) + np.trace(s2))


def test_frechet_identical_inputs():
    x = features(400, 64).astype(np.float64)
    mu, s = x.mean(0), np.cov(x, rowvar=False)
    assert abs(FID.frechet_distance(mu, s, mu, s)) <= 1e-10 * 2 * np.trace(s)


def test_frechet_sample_covariances_against_sqrtm():
    x, y = features(400, 64, seed=1).astype(np.float64), (features(400, 64, seed=2).astype(np.float64)) ** 2
    m1, s1, m2, s2 = x.mean(0), np.cov(x, rowvar=False), y.mean(0), np.cov(y, rowvar=False)
    assert abs(FID.frechet_distance(m1, s1, m2, s2) - sqrtm_distance(m1, s1, m2, s2)) <= 1e-10 * (np.trace(s1) + np.trace(s2))


@pytest.mark.parametrize("N", [20, 24])
def test_frechet_rank_deficient(N):
    """a null direction perturbs a root by the root of the perturbation: D * sqrt(2^-53) of the traces"""
    D = 64
    x, y = features(N, D, seed=3).astype(np.float64), features(N, D, seed=4).astype(np.float64) ** 2
    m1, s1, m2, s2 = x.mean(0), np.cov(x, rowvar=False), y.mean(0), np.cov(y, rowvar=False)
    got, want = FID.frechet_distance(m1, s1, m2, s2), sqrtm_distance(m1, s1, m2, s2)
    scale = np.trace(s1) + np.trace(s2)
    print("rank-deficient N=%d: relative difference %.3g" % (N, abs(got - want) / scale))
    assert np.isfinite(got) and abs(got - want) <= D * np.sqrt(U) * scale


# ---- host checks --------------------------------------------------------------------------------------------------------------------
def test_validation(tmp_path):
    u8 = torch.zeros((2, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="export_images"):
        FID.inception_input(u8.float())
    for bad in (u8[..., :2], torch.zeros((4, 4), dtype=torch.uint8), torch.zeros((1, 1, 2, 4, 4, 3), dtype=torch.uint8), u8.numpy()):
        with pytest.raises(ValueError):
            FID.inception_input(bad)
    for size in (0, 1025, 2.5):
        with pytest.raises(ValueError):
            FID.inception_input(u8, size=size)
    with pytest.raises(ValueError):
        FID.inception_input(torch.zeros((1, 1025, 4, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FID.inception_input(u8)                                          # a host tensor: there is no eager fall-back
    for dims in (0, -1, 2.5):
        with pytest.raises(ValueError):
            FID.FidStatistics(dims)
    with pytest.raises(ValueError):
        FID.FidStatistics(8, capacity=0)
    st = FID.FidStatistics(8)
    for bad in (torch.zeros((3, 8), dtype=torch.float64), torch.zeros((3, 8), dtype=torch.int32), torch.zeros((3, 7)), torch.zeros((3, 8, 2, 1)),
                np.zeros((3, 8), dtype=np.float32)):
        with pytest.raises(ValueError):
            st.update(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.update(torch.zeros((3, 8)))
    with pytest.raises(ValueError, match="at least two"):
        st.finalize()
    with pytest.raises(ValueError):
        FID.fid_statistics_host(np.zeros((1, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        FID.frechet_distance(np.zeros(3), np.eye(3), np.zeros(4), np.eye(4))
    with pytest.raises(ValueError):
        FID.FidStatistics.from_frames(u8.float(), lambda x: x)


def test_npz_round_trip(tmp_path):
    x = features(50, 6).astype(np.float64)
    path = os.path.join(str(tmp_path), "stats.npz")
    np.savez(path, mu=x.mean(0), sigma=np.cov(x, rowvar=False))         # the file fid_score.py:224-227 reads
    st = FID.FidStatistics.load(path)
    mu, sigma = st.finalize()
    assert st.dims == 6 and mu.dtype == sigma.dtype == torch.float64 and mu.device.type == "cpu"
    assert np.array_equal(mu.numpy(), x.mean(0)) and np.array_equal(sigma.numpy(), np.cov(x, rowvar=False))
    again = os.path.join(str(tmp_path), "again.npz")
    st.save(again)
    with np.load(again) as f:
        assert sorted(f.files) == ["mu", "sigma"] and np.array_equal(f["mu"], x.mean(0)) and np.array_equal(f["sigma"], sigma.numpy())
    with pytest.raises(ValueError):
        st.update(torch.zeros((2, 6)))                                   # loaded statistics hold no features
    assert abs(FID.frechet_distance(mu, sigma, *FID.FidStatistics.load(again).finalize())) <= 1e-10 * 2 * float(torch.trace(sigma))
    np.savez(os.path.join(str(tmp_path), "bad.npz"), mu=np.zeros(3), sigma=np.zeros((2, 2)))
    with pytest.raises(ValueError):
        FID.FidStatistics.load(os.path.join(str(tmp_path), "bad.npz"))


def test_abi_rows(pkg):
    N = pkg._native
    bn = importlib.import_module("3d-magic-mirror_amd.build_native")
    assert bn.SOURCES["mm_fid.hip"] == bn.EXACT
    assert N.STRUCT_IDS[43] is N.MMFidInputDesc and N.STRUCT_IDS[44] is N.MMFidStatsDesc
    lib = N.lib()
    assert lib.mm_struct_size(43) == ctypes.sizeof(N.MMFidInputDesc) == 56
    assert lib.mm_struct_size(44) == ctypes.sizeof(N.MMFidStatsDesc) == 48
    assert pkg.FID_SPLIT == N.FID_SPLIT == SPLIT and pkg.inception_input is FID.inception_input and pkg.fid_score is FID.fid_score
    assert pkg.FidStatistics is FID.FidStatistics and pkg.frechet_distance is FID.frechet_distance
    # refusals before any GPU work
    assert lib.mm_fid_input(None, None) == -1 and lib.mm_fid_input(ctypes.byref(N.MMFidInputDesc()), None) == -2
    d = N.MMFidInputDesc()
    d.n, d.H, d.W, d.Ho, d.Wo = 1, 4, 4, 1025, 4
    assert lib.mm_fid_input(ctypes.byref(d), None) == -2
    d.Ho = 2
    assert lib.mm_fid_input(ctypes.byref(d), None) == -1
    rows = np.zeros((6, 4), dtype=np.int32)
    rows[5, 1] = 4                                                       # a tap outside the axis: refused from the host's copy
    buf = (ctypes.c_uint8 * 64)()
    d.frames = d.params = d.out = ctypes.addressof(buf) // 16 * 16 + 16
    d.params_host = rows.ctypes.data
    assert lib.mm_fid_input(ctypes.byref(d), None) == -2
    s = N.MMFidStatsDesc()
    assert lib.mm_fid_stats(None, None) == -1 and lib.mm_fid_stats(ctypes.byref(s), None) == -2
    s.N, s.D = 1, 4
    assert lib.mm_fid_stats_query_workspace(ctypes.byref(s)) == 0 and lib.mm_fid_stats(ctypes.byref(s), None) == -2
    s.N, s.D = 8, 65536
    assert lib.mm_fid_stats_query_workspace(ctypes.byref(s)) == 0 and lib.mm_fid_stats(ctypes.byref(s), None) == -5
    s.N, s.D = SPLIT + 1, 2048                                           # 17 column-sum chunks, then two splits of 528 tiles
    assert lib.mm_fid_stats_query_workspace(ctypes.byref(s)) == 17 * 2048 * 8 + 2 * 528 * 64 * 64 * 8
    assert lib.mm_fid_stats(ctypes.byref(s), None) == -1
    s.x = s.mu = s.sigma = s.workspace = 256
    assert lib.mm_fid_stats(ctypes.byref(s), None) == -3
