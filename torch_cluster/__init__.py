"""Drop-in for the two `torch_cluster` operators IGS uses (igs/models/gs.py:41 `from torch_cluster import fps, knn`,
igs/models/grid_encoder.py:13, main.py:34), backed by the MI355X-native HIP library (igs_amd/csrc/anchors.hip).

Only `knn` and `fps` are defined, with upstream's signatures.  Unsupported cases raise NotImplementedError: cosine=True, points that
are not [N, 3], and dtypes other than float32.  CPU tensors raise RuntimeError (no CPU fallback).  Tie rules, start draws and the
initial distance are documented in INTEGRATION.md ("Semantics that differ").
"""
import torch

from igs_amd import anchors as _A

__all__ = ["knn", "fps"]

# Upstream's CUDA fps: dist = full(N, 5e4); start = (rand(B) * deg).long() on src's device.  Both are recalled from upstream's CUDA
# source, which is not vendored here.
FPS_INIT_DIST = 5e4


def _batch_size(*batches):
    bs = 1
    for b in batches:
        if b is not None and b.numel() > 0:
            bs = max(bs, int(b.max()) + 1)
    return bs


def knn(x, y, k, batch_x=None, batch_y=None, cosine=False, num_workers=1, batch_size=None):
    """For every y[j], the k nearest x[i] of the same example.  Returns [2, E] int64: row 0 the y index (ascending), row 1 the x
    index, ordered by (squared distance, x index) inside a row; queries with fewer than k candidates have fewer entries."""
    if cosine:
        raise NotImplementedError("torch_cluster.knn: cosine=True is not supported on this backend")
    _A.check_points(x, "torch_cluster.knn", "x", gpu=False)
    _A.check_points(y, "torch_cluster.knn", "y", gpu=False)
    k = int(k)
    if not 1 <= k <= _A.KNN_MAX_K:
        raise ValueError(f"torch_cluster.knn: k must be in [1, {_A.KNN_MAX_K}] (got {k})")
    _A.check_gpu(x, "torch_cluster.knn", "x")
    _A.check_gpu(y, "torch_cluster.knn", "y")
    if x.shape[0] == 0 or y.shape[0] == 0:
        return torch.empty(2, 0, dtype=torch.long, device=x.device)
    if batch_size is None:
        batch_size = _batch_size(batch_x, batch_y)
    dev = x.device
    ptr_x = _A.ptr_from_batch(batch_x, x.shape[0], batch_size, dev)
    ptr_y = _A.ptr_from_batch(batch_y, y.shape[0], batch_size, dev)
    idx, _, _ = _A.knn_native(x, y, k, ptr_x, ptr_y)
    mask = idx >= 0
    row = torch.arange(y.shape[0], device=dev).view(-1, 1).expand(-1, k)
    return torch.stack([row.masked_select(mask), idx.masked_select(mask)], 0)


def fps(src, batch=None, ratio=0.5, random_start=True, batch_size=None, ptr=None):
    """Farthest-point sampling of every example: ceil(ratio * n_b) points (float32 arithmetic), global indices in selection order.
    The start is the example's first point, or floor(rand * n_b) with torch.rand on src's device when random_start."""
    _A.check_points(src, "torch_cluster.fps", "src", gpu=False)
    r = torch.as_tensor(1.0 if ratio is None else ratio, dtype=src.dtype)
    if r.numel() == 0 or not bool(((r > 0) & (r <= 1)).all()):
        raise ValueError(f"torch_cluster.fps: ratio must be in (0, 1] (got {ratio})")
    _A.check_gpu(src, "torch_cluster.fps", "src")
    dev = src.device
    r = r.to(dev)
    N = src.shape[0]
    if ptr is not None:
        ptr_vec = torch.as_tensor(ptr, device=dev).long()
    elif batch is not None:
        if batch.numel() != N:
            raise ValueError(f"torch_cluster.fps: batch has {batch.numel()} entries for {N} points")
        if batch_size is None:
            batch_size = _batch_size(batch)
        ptr_vec = _A.ptr_from_batch(batch, N, batch_size, dev).long()
    else:
        ptr_vec = torch.tensor([0, N], device=dev)
    B = ptr_vec.numel() - 1
    deg = ptr_vec[1:] - ptr_vec[:-1]
    out_ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.ceil(deg.to(r.dtype) * r).long().cumsum(0)])
    if random_start:
        start = (torch.rand(B, dtype=src.dtype, device=dev) * deg.to(src.dtype)).long()
    else:
        start = torch.zeros(B, dtype=torch.long, device=dev)
    host = torch.cat([out_ptr[-1:], deg.max().view(1) if B > 0 else out_ptr[-1:]]).cpu()     # the output size (upstream reads it too)
    total, max_n = int(host[0]), int(host[1])
    if total == 0:
        return torch.empty(0, dtype=torch.long, device=dev)
    return _A.fps_native(src, ptr_vec.to(torch.int32), start.to(torch.int32), out_ptr.to(torch.int32), total, max_n, FPS_INIT_DIST)
