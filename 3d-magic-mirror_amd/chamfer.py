"""Chamfer distance with pytorch3d's semantics (pytorch3d.loss.chamfer_distance, defaults: point_reduction='mean',
batch_reduction='mean', no normals), which the reference imports at /root/reference/networks.py:19 and calls at :342,356
and trainer.py:445,469,483.  pytorch3d is absent here (and has no ROCm wheel): parity is against a torch brute force.

The O(N*M) nearest-neighbour search runs in the HIP kernel behind `mm_chamfer_nearest` (both directions, one launch); the loss is
then a gather of the nearest points, and its backward the HIP kernel behind `mm_chamfer_backward` (gradients flow to both clouds
exactly as through knn_points' returned distances).  That backward sums every point's contributions in ascending index, without the
float atomics of the gather's own backward (scatter_add): the gradients are bitwise reproducible and each batch row's are
independent of the other rows.  They are computed in fp32, the precision of the search, and returned in the inputs' dtype."""
import torch
from torch.autograd.function import once_differentiable

from . import _native as N


def nearest_neighbour(x, y):
    """x (B,N,3), y (B,M,3) device tensors -> (squared distance (B,N), index (B,N) int64) of the nearest y for every x."""
    N.require_device(x, y)
    xc, yc = x.detach().float().contiguous(), y.detach().float().contiguous()
    B, n, _ = xc.shape
    m = yc.shape[1]
    dist = torch.empty((B, n), device=x.device, dtype=torch.float32)
    idx = torch.empty((B, n), device=x.device, dtype=torch.int32)
    N.call("mm_nearest_neighbour", x.device, B, n, m, N.ptr(xc), N.ptr(yc), N.ptr(dist), N.ptr(idx))
    return dist, idx.long()


def _nearest_both_i32(x, y):
    """(x, y as contiguous fp32, index (B,N) int32 of the nearest y for every x, index (B,M) int32 of the nearest x for every y)."""
    N.require_device(x, y)
    xc, yc = x.detach().float().contiguous(), y.detach().float().contiguous()
    B, n, _ = xc.shape
    m = yc.shape[1]
    dist = torch.empty((B, n + m), device=x.device, dtype=torch.float32)
    idx = torch.empty((B * (n + m),), device=x.device, dtype=torch.int32)
    dx, dy = dist.view(-1)[:B * n], dist.view(-1)[B * n:]
    ix, iy = idx[:B * n], idx[B * n:]
    N.call("mm_chamfer_nearest", x.device, B, n, m, N.ptr(xc), N.ptr(yc), N.ptr(dx), N.ptr(ix), N.ptr(dy), N.ptr(iy))
    return xc, yc, ix.view(B, n), iy.view(B, m)


def nearest_both(x, y):
    """Both directions in ONE launch (mm_chamfer_nearest): (index (B,N) of the nearest y for every x, index (B,M) of the nearest x for every y)."""
    _, _, ix, iy = _nearest_both_i32(x, y)
    return ix.long(), iy.long()


class _ChamferFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        xc, yc, ix, iy = _nearest_both_i32(x, y)
        ixl, iyl = ix.long(), iy.long()
        cham_x = (x - torch.gather(y, 1, ixl.unsqueeze(-1).expand(-1, -1, 3))).pow(2).sum(-1)     # (B,N)
        cham_y = (y - torch.gather(x, 1, iyl.unsqueeze(-1).expand(-1, -1, 3))).pow(2).sum(-1)     # (B,M)
        ctx.save_for_backward(xc, yc, ix, iy)
        ctx.dtypes = (x.dtype, y.dtype)
        return cham_x.mean(1).mean(0) + cham_y.mean(1).mean(0)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        xc, yc, ix, iy = ctx.saved_tensors
        B, n, m = xc.shape[0], xc.shape[1], yc.shape[1]
        g = grad_loss.detach().reshape(1).to(device=xc.device, dtype=torch.float32).contiguous()    # (read by the kernel: no sync)
        gx, gy = torch.empty_like(xc), torch.empty_like(yc)
        N.call("mm_chamfer_backward", xc.device, B, n, m, N.ptr(xc), N.ptr(yc), N.ptr(ix), N.ptr(iy), N.ptr(g), N.ptr(gx), N.ptr(gy))
        return (gx.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None,
                gy.to(ctx.dtypes[1]) if ctx.needs_input_grad[1] else None)


def chamfer_distance(x, y):
    """Returns (loss, None) like pytorch3d: mean_b [ mean_i min_j |x_i - y_j|^2 + mean_j min_i |x_i - y_j|^2 ]."""
    if x.dim() != 3 or y.dim() != 3 or x.shape[0] != y.shape[0] or x.shape[2] != 3 or y.shape[2] != 3:
        raise ValueError("chamfer_distance expects (B,N,3) and (B,M,3)")
    return _ChamferFn.apply(x, y), None
