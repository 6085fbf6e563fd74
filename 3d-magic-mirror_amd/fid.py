"""FID of device frames without a file or a host round trip: host side of ``mm_fid_input`` and ``mm_fid_stats`` (csrc/mm_fid.hip).

The reference judges a checkpoint by SSIM, ``1 - mask_iou`` and FID of the images it saved, and keeps ``best_ckpt.pth`` by FID alone
(trainer.py:771-836, :938-976, test.py:430-463).  Per evaluation it calls ``calculate_fid_given_paths`` three times with the same ``ori``
directory; each call opens every file on the host, uploads batches of 64, resizes to 299 x 299, runs InceptionV3, copies the features back,
takes ``np.mean`` / ``np.cov`` of an (N, 2048) float64 array and ends with ``scipy.linalg.sqrtm`` of a 2048 x 2048 product
(fid_score.py:71-255, inception.py:129-163).  Here

    inception_input    uint8 device frames -> the network's (n,3,299,299) float32 batch, one launch
    FidStatistics      features appended on the device; ``finalize`` -> float64 (mu, sigma) from four launches, bit-identical run to run
    frechet_distance   the distance from two symmetric eigen-decompositions (no complex matrix root, no ``eps`` retry)
    fid_score          the three composed; either side may be a finalized ``FidStatistics``, so ``ori`` is scored once for all three FIDs

The network is a dense convolution stack and stays stock PyTorch-ROCm; ``model`` is any callable.  Nothing here is differentiable.

The arithmetic of ``inception_input``, every step rounded in fp32 and nothing contracted (``inception_input_host`` restates it in numpy):
``t = float(byte) / 255.0f`` by IEEE division; horizontally ``h = w0x * t[i0x] + w1x * t[i1x]`` on the two source rows; vertically
``v = w0y * h[i0y] + w1y * h[i1y]``; then ``2 * v - 1``.  The taps are ``frames.resize_taps(n_in, size, coords=np.float64)``: torch's
bilinear resize with align_corners=False as it resizes a float64 tensor, each weight rounded to fp32 once (the fp32 kernel's coordinate
alone is 6e-5 off at these sizes; the result is held to 1e-6 of the float64 composition); a tap it drops has weight 0.  The order of the statistics is in ``fid_statistics_host`` and DESIGN.md."""
import ctypes

import numpy as np
import torch

from . import _native as N
from .frames import resize_taps

FID_SPLIT = N.FID_SPLIT              # rows of one split of the Gram matrix (MM_FID_SPLIT)
FID_SUM_ROWS = N.FID_SUM_ROWS        # rows of one column-sum chunk (MM_FID_SUM_ROWS)
FID_TILE = 64                        # the Gram matrix's macro-tile (MM_FID_TILE): only tiles on or above the diagonal are computed
FID_MAX_SIDE = N.FID_MAX_SIDE

# (H, W, size, device) -> (Ho, Wo, pinned host rows, device rows).  Resident: the device rows' upload has finished when the call that
# made the entry returns, nothing writes them afterwards, so calls on any stream may share them (one host wait per new key, none after).
_TABLES = {}


def _axis_rows(n_in, n_out):
    """(n_out,4) int32 {i0, i1, w0 bits, w1 bits} of one axis: ``resize_taps`` as exactly two taps (a dropped tap: weight 0, i1 clamped);
    n_out None is no resize, every output its own input with weight 1"""
    r = np.zeros((n_in if n_out is None else n_out, 4), dtype=np.int32)
    if n_out is None:
        r[:, 0] = r[:, 1] = np.arange(n_in)
        w = np.zeros((n_in, 2), dtype=np.float32)
        w[:, 0] = 1.0
    else:
        start, count, taps = resize_taps(n_in, n_out, coords=np.float64)
        if int(count.max()) > 2:
            raise RuntimeError("resize_taps gave %d taps for a bilinear axis" % int(count.max()))
        r[:, 0] = start.numpy()
        r[:, 1] = np.minimum(r[:, 0] + 1, n_in - 1)
        w = np.ascontiguousarray(taps.numpy()[:, :2])
    r[:, 2:] = w.view(np.int32)
    return r


def _check_sizes(H, W, size):
    if size is not None and (isinstance(size, bool) or int(size) != size):
        raise ValueError("size must be an int or None, got %r" % (size,))
    if not (1 <= H <= FID_MAX_SIDE and 1 <= W <= FID_MAX_SIDE) or (size is not None and not 1 <= size <= FID_MAX_SIDE):
        raise ValueError("H, W and size must lie in 1..%d, got H %d, W %d, size %r" % (FID_MAX_SIDE, H, W, size))


def lower_inception_input(H, W, size=299):
    """The call's table, host arithmetic only: (Ho, Wo, rows) with rows (Wo + Ho, 4) int32, the rows of x then of y as MMFidInputDesc
    takes them.  ValueError for H, W or size outside 1..FID_MAX_SIDE."""
    H, W = int(H), int(W)
    _check_sizes(H, W, size)
    S = None if size is None else int(size)
    return (H if S is None else S), (W if S is None else S), np.concatenate([_axis_rows(W, S), _axis_rows(H, S)])


def inception_input_host(frames, size=299, normalize=True):
    """``inception_input`` restated in numpy, in the kernel's order: (n,H,W,3) or (H,W,3) uint8 array -> (n,3,S,S) float32"""
    f = np.asarray(frames)
    f = f[None] if f.ndim == 3 else f
    Ho, Wo, rows = lower_inception_input(f.shape[1], f.shape[2], size)
    xr, yr = rows[:Wo], rows[Wo:]
    t = (np.arange(256, dtype=np.float32) / np.float32(255.0))[f]                       # (n,H,W,3)
    w0x, w1x = xr[:, 2].copy().view(np.float32)[None, None, :, None], xr[:, 3].copy().view(np.float32)[None, None, :, None]
    h = w0x * t[:, :, xr[:, 0]] + w1x * t[:, :, xr[:, 1]]                               # (n,H,Wo,3)
    w0y, w1y = yr[:, 2].copy().view(np.float32)[None, :, None, None], yr[:, 3].copy().view(np.float32)[None, :, None, None]
    v = w0y * h[:, yr[:, 0]] + w1y * h[:, yr[:, 1]]                                     # (n,Ho,Wo,3)
    if normalize:
        v = np.float32(2.0) * v - np.float32(1.0)
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2)).astype(np.float32, copy=False)


def _check_frames(frames):
    if not torch.is_tensor(frames):
        raise ValueError("frames must be a uint8 tensor (n,H,W,3), got %s" % type(frames))
    if frames.dtype != torch.uint8:
        raise ValueError("frames must be uint8 (n,H,W,3), got %s: export_images makes 8-bit frames from float renders" % frames.dtype)
    if frames.dim() not in (3, 4) or frames.shape[-1] != 3 or min(frames.shape) < 1:
        raise ValueError("frames must have shape (n,H,W,3) or (H,W,3), got %s" % (tuple(frames.shape),))


def inception_input(frames, size=299, normalize=True, out=None):
    """The Inception network's input batch from 8-bit device frames: (n,H,W,3) uint8 (one (H,W,3) frame is n = 1), as ``export_images``,
    ``composite_frames`` and ``jpeg_roundtrip`` leave them -> contiguous (n,3,size,size) float32: ``v / 255``,
    ``F.interpolate(x, (size, size), mode='bilinear', align_corners=False)``, ``2 x - 1`` (fid_score.py:95-105, inception.py:143-152).

    size       the side of the output, 1..1024; None skips the resize (the output is (n,3,H,W))
    normalize  False skips ``2 x - 1``; with size=None that is the [0,1] batch a default-flag ``InceptionV3`` expects
    out        a float32 contiguous device tensor of the result's shape to write into

    Any byte alignment; other strides go through ``.contiguous()``.  Float input is refused: ``export_images`` makes the bytes.  One launch on
    the current stream; nothing synchronises, except that the first call of an (H, W, size, device) waits once for its table's upload
    (``_TABLES``: finished on return, read-only afterwards, shared by calls on any stream).  H and W in 1..1024."""
    _check_frames(frames)
    H, W = frames.shape[-3], frames.shape[-2]
    _check_sizes(H, W, size)
    N.require_device(frames)
    dev = frames.device
    key = (H, W, size, dev)
    tables = _TABLES.get(key)                                    # (Ho, Wo, pinned host rows, device rows): lowered and uploaded once
    if tables is None:
        Ho, Wo, rows = lower_inception_input(H, W, size)
        if len(_TABLES) >= 64:
            _TABLES.clear()
        tables = _TABLES[key] = (Ho, Wo) + N.upload_int32(rows, dev, wait=True)      # resident: finished before any stream may share it
    Ho, Wo = tables[:2]
    frames = frames.detach().contiguous()
    n = 1 if frames.dim() == 3 else frames.shape[0]
    shape = (n, 3, Ho, Wo)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != dev or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of shape %s on %s" % (shape, dev))
    d = N.MMFidInputDesc()
    d.n, d.H, d.W, d.Ho, d.Wo, d.normalize = n, H, W, Ho, Wo, int(bool(normalize))
    d.frames, d.params_host, d.params, d.out = N.ptr(frames), ctypes.c_void_p(tables[2].data_ptr()), N.ptr(tables[3]), N.ptr(out)
    N.call("mm_fid_input", dev, d)
    return out


def fid_statistics_host(features, fault=None):
    """``FidStatistics.finalize`` restated in numpy with the kernels' splits and order: (N,D) float32 -> (mu (D,), sigma (D,D)) float64.

    Column sums: float64, chunks of FID_SUM_ROWS rows added row by row, the chunks then added ascending; mu = sum / N.  Gram matrix: per split
    of FID_SPLIT rows, groups of four rows ascending, each row's product of the centred float64 values added to the split's accumulator
    (a row beyond N is zero); the splits added ascending; one division by N - 1; the upper triangle mirrored.

    fault, for the tests that show the cases catch a wrong kernel: "div_n" divides by N; "drop_tail" drops the last partial group of four
    rows; "uncentred" leaves mu out of the moments; "no_mirror" leaves the lower triangle unwritten."""
    x = np.asarray(features)
    if x.dtype != np.float32 or x.ndim != 2:
        raise ValueError("features must be a (N,D) float32 array")
    n, D = x.shape
    if n < 2:
        raise ValueError("the covariance needs at least two rows, got %d" % n)
    total = np.zeros(D, dtype=np.float64)
    for c0 in range(0, n, FID_SUM_ROWS):
        s = np.zeros(D, dtype=np.float64)
        for r in range(c0, min(n, c0 + FID_SUM_ROWS)):
            s = s + x[r].astype(np.float64)
        total = total + s
    mu = total / np.float64(n)
    centre = np.zeros(D) if fault == "uncentred" else mu
    rows = n - n % 4 if fault == "drop_tail" else n
    gram = np.zeros((D, D), dtype=np.float64)
    for s0 in range(0, n, FID_SPLIT):
        acc = np.zeros((D, D), dtype=np.float64)
        for r in range(s0, min(rows, s0 + FID_SPLIT)):
            xc = x[r].astype(np.float64) - centre
            acc = acc + xc[:, None] * xc[None, :]
        gram = gram + acc
    upper = np.triu(gram / np.float64(n if fault == "div_n" else n - 1))
    sigma = upper if fault == "no_mirror" else upper + np.triu(upper, 1).T
    return mu, sigma


class FidStatistics:
    """The running feature statistics of one image set: ``update`` appends (b,D) or (b,D,1,1) device features, ``finalize`` gives float64
    ``(mu (D,), sigma (D,D))`` on the device with the meaning of ``np.mean(act, axis=0)`` and ``np.cov(act, rowvar=False)`` of the float64
    copy of the features (fid_score.py:131-138): centred first, divided by N - 1.

    dims      D, the feature width (the reference's InceptionV3 blocks give 64, 192, 768 or 2048; any D >= 1 is taken)
    capacity  rows to allocate at once; without it the buffer starts at 1024 rows and doubles

    Features are float32; float16 and bfloat16 are widened exactly; float64 and integers are refused.  ``update`` never synchronises: the
    row count comes from shapes.  ``finalize`` is four launches without float atomics: bit-identical from run to run, sigma exactly
    symmetric (fid_statistics_host has the order).  Fewer than two rows raise ValueError (the reference would return NaN).  ``save`` / ``load``
    use the ``.npz`` with keys ``mu`` and ``sigma`` that fid_score.py:224-227 reads."""

    def __init__(self, dims, capacity=None):
        if isinstance(dims, bool) or int(dims) != dims or int(dims) < 1:
            raise ValueError("dims must be a positive int, got %r" % (dims,))
        if capacity is not None and (int(capacity) != capacity or int(capacity) < 1):
            raise ValueError("capacity must be a positive int, got %r" % (capacity,))
        self.dims = int(dims)
        self.n = 0
        self.mu = self.sigma = None
        self._capacity = None if capacity is None else int(capacity)
        self._buf = None

    def update(self, features):
        if not torch.is_tensor(features):
            raise ValueError("features must be a tensor (b,%d) or (b,%d,1,1), got %s" % (self.dims, self.dims, type(features)))
        if features.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError("features must be float32, float16 or bfloat16, got %s" % features.dtype)
        s = tuple(features.shape)
        if not ((len(s) == 2 or (len(s) == 4 and s[2:] == (1, 1))) and s[1] == self.dims):
            raise ValueError("features must have shape (b,%d) or (b,%d,1,1), got %s" % (self.dims, self.dims, s))
        if self.mu is not None and self._buf is None:
            raise ValueError("these statistics were loaded or given as (mu, sigma): there are no features to add to")
        N.require_device(features)
        if self._buf is not None and features.device != self._buf.device:
            raise ValueError("features are on %s, the buffer on %s" % (features.device, self._buf.device))
        b = s[0]
        if b == 0:
            return self
        need = self.n + b
        if self._buf is None or need > self._buf.shape[0]:
            cap = self._capacity or 1024 if self._buf is None else self._buf.shape[0]
            while cap < need:
                cap *= 2
            buf = torch.empty((cap, self.dims), dtype=torch.float32, device=features.device)
            if self.n:
                buf[:self.n].copy_(self._buf[:self.n])
            self._buf = buf
        self._buf[self.n:need].copy_(features.detach().reshape(b, self.dims))        # (the copy widens float16 / bfloat16 exactly)
        self.n = need
        self.mu = self.sigma = None
        return self

    def finalize(self):
        if self.mu is not None:
            return self.mu, self.sigma
        if self.n < 2:
            raise ValueError("the covariance needs at least two feature rows, got %d" % self.n)
        dev = self._buf.device
        d = N.MMFidStatsDesc()
        d.N, d.D, d.x = self.n, self.dims, N.ptr(self._buf)
        mu = torch.empty((self.dims,), dtype=torch.float64, device=dev)
        sigma = torch.empty((self.dims, self.dims), dtype=torch.float64, device=dev)
        d.mu, d.sigma = N.ptr(mu), N.ptr(sigma)
        if N.fn("mm_fid_stats_query_workspace")(d) == 0:
            raise ValueError("statistics of %d rows of %d features are beyond the kernels' grids" % (self.n, self.dims))
        ws = N.workspace("mm_fid_stats_query_workspace", d, dev)
        N.call("mm_fid_stats", dev, d)
        del ws                                                                        # (stream-ordered: the allocator reuses it after the call)
        self.mu, self.sigma = mu, sigma
        return mu, sigma

    def save(self, path):
        """write ``mu`` and ``sigma`` as the ``.npz`` fid_score.py reads (one blocking copy to the host)"""
        mu, sigma = self.finalize()
        with open(path, "wb") as f:
            np.savez(f, mu=mu.cpu().numpy(), sigma=sigma.cpu().numpy())

    @classmethod
    def load(cls, path, device=None):
        """the statistics of an ``.npz`` with keys ``mu`` and ``sigma``, finalized, as float64 tensors on ``device`` (the host by default)"""
        with np.load(path) as f:
            mu, sigma = np.asarray(f["mu"], dtype=np.float64), np.asarray(f["sigma"], dtype=np.float64)
        if mu.ndim != 1 or sigma.shape != (mu.shape[0], mu.shape[0]) or mu.shape[0] < 1:
            raise ValueError("%s holds mu %s and sigma %s, not (D,) and (D,D)" % (path, mu.shape, sigma.shape))
        st = cls(mu.shape[0])
        st.mu, st.sigma = torch.from_numpy(mu).to(device or "cpu"), torch.from_numpy(sigma).to(device or "cpu")
        return st

    @classmethod
    def from_frames(cls, frames, model, batch_size=64, as_saved=False, quality=100, dims=None):
        """The statistics of uint8 device frames (...,H,W,3) under ``model``, finalized: batches of ``batch_size`` (the tail included, as
        fid_score.py:108 includes it) through ``inception_input``, ``model`` under ``no_grad`` and ``update``.  as_saved first passes the
        frames through ``jpeg_roundtrip(frames, quality)``: the reference scores files.  dims defaults to the first batch's feature width."""
        if torch.is_tensor(frames) and frames.dim() > 4:
            frames = frames.reshape((-1,) + tuple(frames.shape[-3:]))
        _check_frames(frames)
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive, got %r" % (batch_size,))
        frames = frames.reshape((-1,) + tuple(frames.shape[-3:]))
        if as_saved:
            from .jpeg import jpeg_roundtrip
            frames = jpeg_roundtrip(frames, quality)
        st = None
        with torch.no_grad():
            for i in range(0, frames.shape[0], int(batch_size)):
                feat = model(inception_input(frames[i:i + int(batch_size)]))
                if st is None:
                    st = cls(feat.shape[1] if dims is None else dims, capacity=frames.shape[0])
                st.update(feat)
        st.finalize()
        return st


def _f64(x, device):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x))
    return t.detach().to(device=device, dtype=torch.float64)


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """``|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2)`` (fid_score.py:141-195) in float64, as a Python float.  Torch tensors of either
    device or numpy arrays; it runs where ``sigma1`` lives (the device for ``FidStatistics.finalize`` results, the host for arrays).

    For symmetric positive semi-definite inputs ``tr sqrt(S1 S2) = sum sqrt(max(eig(R S2 R), 0))`` with ``R = S1^(1/2)`` from ``eigh``: two
    symmetric eigen-decompositions through ``torch.linalg``, no complex matrix root.  The result is not clamped, and there is no ``eps``
    retry: the symmetric form does not produce the non-finite product fid_score.py:178-183 retries on."""
    device = sigma1.device if torch.is_tensor(sigma1) else torch.device("cpu")
    mu1, sigma1, mu2, sigma2 = (_f64(t, device) for t in (mu1, sigma1, mu2, sigma2))
    D = mu1.shape[0] if mu1.dim() == 1 else -1
    if D < 1 or mu2.shape != (D,) or sigma1.shape != (D, D) or sigma2.shape != (D, D):
        raise ValueError("mu must be (D,) and sigma (D,D) on both sides, got %s, %s, %s, %s"
                         % tuple(tuple(t.shape) for t in (mu1, sigma1, mu2, sigma2)))
    w, V = torch.linalg.eigh(sigma1)
    R = (V * w.clamp_min(0.0).sqrt()) @ V.T
    M = R @ sigma2 @ R
    ev = torch.linalg.eigvalsh((M + M.T) * 0.5)
    diff = mu1 - mu2
    return float(diff.dot(diff) + torch.trace(sigma1) + torch.trace(sigma2) - 2.0 * ev.clamp_min(0.0).sqrt().sum())


def fid_score(a, b, model, batch_size=64, as_saved=False, quality=100):
    """FID of two image sets under ``model``: each of a and b is uint8 device frames (...,H,W,3) or a finalized ``FidStatistics`` (so the
    ``ori`` side of the reference's three FIDs is scored once).  model: any callable from (b,3,299,299) float32 in [-1,1] to (b,D) or
    (b,D,1,1); for pytorch-fid ``lambda x: net(x)[0]`` with ``net = InceptionV3([3], resize_input=False, normalize_input=False)``
    (INTEGRATION 2r).  batch_size, as_saved, quality: ``FidStatistics.from_frames``.  A Python float, after the one blocking read of it."""
    sides = [s if isinstance(s, FidStatistics) else FidStatistics.from_frames(s, model, batch_size, as_saved, quality) for s in (a, b)]
    (mu1, s1), (mu2, s2) = sides[0].finalize(), sides[1].finalize()
    return frechet_distance(mu1, s1, mu2, s2)
