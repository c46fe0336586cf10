"""Restatement of simple-knn's distCUDA2 (include/igs_rast.h: igs_knn_mean_dist2) for the kNN tests: a float64 brute force, a float32
one with upstream's rounding and FLT_MAX slots, and the closed forms of create_from_pcd.

out[i] = (b0 + b1 + b2) / 3.0f, b0 <= b1 <= b2 the three smallest squared distances |p_i - p_j|^2 over j != i (by index: duplicates
count, at distance 0).  Slots without a neighbour (N <= 3) hold FLT_MAX and the sum runs left to right in float32.  The simple-knn
source is not vendored here; the N <= 3 rule is pinned from a reading of upstream's `best[3] = {FLT_MAX, ...}` and
`(best[0] + best[1] + best[2]) / 3.0f`, not from reference output."""
import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)
SH_C0 = 0.28209479177387814


def brute_f64(x, queries=None, chunk=16):
    """float64 truth: (b0 + b1 + b2) / 3 for the rows `queries` (default: all) of the [N, 3] tensor x, N >= 4, on x's device."""
    x = torch.as_tensor(x).double()
    N = x.shape[0]
    q_idx = torch.arange(N, device=x.device) if queries is None else torch.as_tensor(queries, device=x.device)
    out = torch.empty(q_idx.shape[0], dtype=torch.float64, device=x.device)
    for a in range(0, q_idx.shape[0], chunk):
        qi = q_idx[a:a + chunk]
        q = x[qi]
        d = (q[:, None, 0] - x[None, :, 0]) ** 2
        d += (q[:, None, 1] - x[None, :, 1]) ** 2
        d += (q[:, None, 2] - x[None, :, 2]) ** 2
        d[torch.arange(qi.shape[0], device=x.device), qi] = float("inf")
        out[a:a + chunk] = torch.topk(d, 3, dim=1, largest=False).values.sum(dim=1) / 3.0
    return out


def restate_f32(x):
    """float32 restatement (numpy, O(N^2) memory: small N): squared distances rounded per operation, FLT_MAX slots, left-to-right
    sum, / 3.0f.  Bit-equal to the kernel wherever the distances are exact in float32 (integer lattices)."""
    x = np.asarray(x, dtype=np.float32)
    N = x.shape[0]
    d = np.zeros((N, N), dtype=np.float32)
    for k in range(3):
        t = (x[:, None, k] - x[None, :, k]).astype(np.float32)
        d = (d + t * t).astype(np.float32)
    np.fill_diagonal(d, np.inf)
    best = np.full((N, 3), np.float32(FLT_MAX), dtype=np.float32)
    k = min(3, N - 1)
    if k > 0:
        best[:, :k] = np.sort(d, axis=1)[:, :k]
    with np.errstate(over="ignore"):                    # N <= 2: FLT_MAX + FLT_MAX = inf, as upstream
        s = (best[:, 0] + best[:, 1]).astype(np.float32)
        s = (s + best[:, 2]).astype(np.float32)
    return (s / np.float32(3.0)).astype(np.float32)


def lattice(n, dims=3, spacing=1.0):
    """n^dims integer lattice points (z = 0 for dims == 2), float32 [n^dims, 3]."""
    axes = [np.arange(n, dtype=np.float32) * np.float32(spacing)] * dims + [np.zeros(1, dtype=np.float32)] * (3 - dims)
    g = np.meshgrid(*axes, indexing="ij")
    return np.stack([a.ravel() for a in g], axis=1).astype(np.float32)


def create_from_pcd(xyz, rgb, dist2, max_sh_degree=3):
    """create_from_pcd (RaDe-GS scene/gaussian_model.py:316-340) given distCUDA2's output, as the raw dict of load_start_gaussians."""
    P, K = xyz.shape[0], (max_sh_degree + 1) ** 2
    shs = torch.zeros((P, K, 3), dtype=torch.float32, device=xyz.device)
    shs[:, 0] = (rgb.float() - 0.5) / SH_C0
    scaling = torch.log(torch.sqrt(torch.clamp_min(dist2, 0.0000001)))[..., None].repeat(1, 3)
    rotation = torch.zeros((P, 4), dtype=torch.float32, device=xyz.device)
    rotation[:, 0] = 1
    o = 0.1 * torch.ones((P, 1), dtype=torch.float32, device=xyz.device)
    return dict(xyz=xyz.float(), rotation=rotation, shs=shs, opacity=torch.log(o / (1 - o)), scaling=scaling)
