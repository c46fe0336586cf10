"""The anchor graph of IGS's AGM-Net on the MI355X-native library (igs_amd/csrc/anchors.hip, include/igs_rast.h).

igs/models/gs.py get_mask_fpsample runs, per frame and per Gaussian set: select_points_bbox, a CPU farthest-point sampling of the
in-box points (fpsample.bucket_fps_kdline_sampling), torch_cluster.knn of every in-box point against the anchors, and softmax weights
of the distances.  `anchor_graph` is that function on the device; `knn_index` is the renderer-side neighbour search (gs.py:805).  The
torch_cluster and fpsample drop-ins (repository root) use the helpers below.

Differences from the reference function: `anchor_idx` holds device int64 tensors rather than numpy arrays, and the FPS starts are
drawn with numpy's global generator (`np.random.randint`, seedable with `np.random.seed`) when `start_idx` is None, as the fpsample
drop-in does.
"""
import math

import numpy as np
import torch

from ._cabi import ext as _ext

KNN_MAX_K = 100                        # IGS_KNN_QUERY_MAX_K (torch_cluster refuses k > 100 as well)
MAX_EXAMPLE_POINTS = 1 << 22           # IGS_FPS_MAX_EXAMPLE_POINTS
MAX_POINTS = 1 << 26                   # IGS_ANCHOR_MAX_POINTS
WEIGHT_SCALE = 10.0                    # gs.py:1009 weights = softmax(-10 * dist)


def check_points(t, fn, name, gpu=True):
    """float32 [N, 3] on a GPU; the unsupported cases raise NotImplementedError, a CPU tensor RuntimeError (as distCUDA2).
    gpu=False leaves the device to check_gpu (argument refusals come before the device test)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{fn}: {name} must be a torch.Tensor (got {type(t).__name__})")
    if t.dim() != 2 or t.shape[1] != 3:
        raise NotImplementedError(f"{fn}: only 3-D points ([N, 3]) are supported ({name} has shape {list(t.shape)})")
    if t.dtype != torch.float32:
        raise NotImplementedError(f"{fn}: only float32 points are supported ({name} is {t.dtype})")
    if t.shape[0] > MAX_POINTS:
        raise RuntimeError(f"{fn}: {t.shape[0]} points is more than the supported {MAX_POINTS}")
    if gpu:
        check_gpu(t, fn, name)


def check_gpu(t, fn, name):
    if not t.is_cuda:
        raise RuntimeError(f"{fn}: {name} must be on a GPU (no CPU fallback)")


def ptr_from_batch(batch, n, batch_size, device):
    """[batch_size + 1] int32 offsets of the examples of a sorted vector of example ids (any integer or floating dtype)."""
    if batch is None:
        return torch.tensor([0, n], dtype=torch.int32, device=device)
    b = torch.as_tensor(batch).to(device=device)
    if b.numel() != n:
        raise ValueError(f"batch has {b.numel()} entries for {n} points")
    b = b.long() if b.dtype != torch.int64 else b
    return torch.searchsorted(b.contiguous(), torch.arange(batch_size + 1, device=device, dtype=torch.int64)).to(torch.int32)


def knn_native(x, y, k, ptr_x, ptr_y, with_d2=False, weight_scale=None):
    """(index into x [Ny, k] int64 with -1 padding, d2 [Ny, k] or None, weights [Ny, k] or None): the k nearest x of each y of
    the same example, ordered by (d2, index); a candidate counts only if d2 < 1e10."""
    return _ext().anchors_knn(x, y, ptr_x, ptr_y, int(k), bool(with_d2), weight_scale)


def fps_native(xyz, ptr, start, out_ptr, total, max_n, init_d2):
    """Vanilla FPS of every example: `total` int64 indices into xyz, example b's at out_ptr[b]..out_ptr[b + 1] in selection order."""
    if max_n > MAX_EXAMPLE_POINTS:
        raise RuntimeError(f"fps: an example of {max_n} points is more than the supported {MAX_EXAMPLE_POINTS}")
    return _ext().anchors_fps(xyz, ptr, start, out_ptr, int(total), int(max_n), float(init_d2))


def bbox_select(xyz, ptr, box):
    """select_points_bbox of B examples at once: (in-box xyz [N, 3], index inside the example [N] int64, counts [B] int32)."""
    return _ext().anchors_bbox_select(xyz, ptr, box)


def knn_index(anchors, points, batch_y=None, k=8, weight_scale=WEIGHT_SCALE):
    """The renderer-side neighbour search of gs.py:795-810: anchors [B, A, 3], points [N, 3] (example ids `batch_y`, sorted, any
    dtype; None: one example).  Returns (row, col, weights [N, k, 1]) where col indexes the flattened anchors [B * A]."""
    B, A = anchors.shape[0], anchors.shape[1]
    flat = anchors.reshape(B * A, 3)
    check_points(flat, "knn_index", "anchors")
    check_points(points, "knn_index", "points")
    if not 1 <= k <= min(KNN_MAX_K, A):
        raise ValueError(f"knn_index: k must be in [1, min(100, anchors per example)] (got {k})")
    dev = points.device
    ptr_x = torch.arange(B + 1, device=dev, dtype=torch.int32) * A
    ptr_y = ptr_from_batch(batch_y, points.shape[0], B, dev)
    idx, _, w = knn_native(flat, points, k, ptr_x, ptr_y, weight_scale=weight_scale)
    row = torch.arange(points.shape[0], device=dev).repeat_interleave(k)
    return row, idx.reshape(-1), w.unsqueeze(-1)


def anchor_graph(xyz_list, bbox, anchor_size=8192, k=8, start_idx=None):
    """get_mask_fpsample (igs/models/gs.py:966-1011) on the device.  xyz_list: B tensors [N_b, 3] (the Gaussians' get_xyz), bbox:
    [B, 2, 3] (lo, hi).  Returns (anchor_points [B, A, 3], masks (B int64 index tensors), weights [sum N_in, k, 1],
    (row, col, batch_x int64, batch_y float32), anchor_idx (B device int64 tensors)).

    One host read: the in-box counts, which the output shapes need.  An example with fewer than `anchor_size` in-box points raises
    ValueError.  start_idx: None (np.random.randint per example, as the fpsample drop-in) or B start indices into the in-box points."""
    xyz_list = list(xyz_list)
    B = len(xyz_list)
    if B < 1:
        raise ValueError("anchor_graph: no examples")
    for i, t in enumerate(xyz_list):
        check_points(t, "anchor_graph", f"xyz_list[{i}]")
    if not 1 <= k <= min(KNN_MAX_K, anchor_size):
        raise ValueError(f"anchor_graph: k must be in [1, min(100, anchor_size)] (got {k})")
    dev = xyz_list[0].device
    sizes = [int(t.shape[0]) for t in xyz_list]
    xyz = torch.cat([t.detach() for t in xyz_list], 0) if B > 1 else xyz_list[0].detach()
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    box = torch.as_tensor(bbox if not isinstance(bbox, (list, tuple)) else torch.stack([torch.as_tensor(b) for b in bbox]))
    box = box.to(device=dev, dtype=torch.float32).reshape(B, 2, 3).contiguous()

    pxyz, pidx, count = bbox_select(xyz, ptr, box)
    counts = count.cpu().tolist()                               # the one host read
    for b, c in enumerate(counts):
        if c < anchor_size:
            raise ValueError(f"anchor_graph: example {b} has {c} points in its box, fewer than anchor_size = {anchor_size}")
    total = sum(counts)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    masks = [pidx[offs[b]:offs[b + 1]] for b in range(B)]
    points = pxyz[:total]

    if start_idx is None:
        starts = [int(np.random.randint(c)) for c in counts]
    else:
        starts = [int(s) for s in start_idx]
        if len(starts) != B or any(not 0 <= s < c for s, c in zip(starts, counts)):
            raise ValueError("anchor_graph: start_idx must hold one index per example inside its in-box points")
    ptr_in = torch.tensor(offs, dtype=torch.int32, device=dev)
    out_ptr = torch.arange(B + 1, device=dev, dtype=torch.int32) * anchor_size
    sel = fps_native(points, ptr_in, torch.tensor(starts, dtype=torch.int32, device=dev), out_ptr, B * anchor_size, max(counts),
                     math.inf)                                   # fpsample: initial cur = +inf
    anchor_points = points[sel].view(B, anchor_size, 3)
    local = (sel.view(B, anchor_size) - ptr_in[:-1, None].long())
    anchor_idx = [local[b] for b in range(B)]

    idx, _, w = knn_native(anchor_points.view(B * anchor_size, 3), points, k, out_ptr, ptr_in, weight_scale=WEIGHT_SCALE)
    row = torch.arange(total, device=dev).repeat_interleave(k)
    col = idx.reshape(-1)
    weights = w.unsqueeze(-1)
    batch_x = torch.arange(B, device=dev).repeat_interleave(anchor_size)
    batch_y = torch.repeat_interleave(torch.arange(B, dtype=torch.float32, device=dev),
                                      torch.tensor(counts, device=dev))
    return anchor_points, masks, weights, (row, col, batch_x, batch_y), anchor_idx
