"""Restatement of the anchor-graph semantics (include/igs_rast.h: igs_bbox_select, igs_fps, igs_knn_query; the torch_cluster and
fpsample drop-ins) for the anchor tests.

Distances are float32 squared distances dx*dx + dy*dy + dz*dz of float32 differences.  The kernels evaluate them as
fma(dz, dz, fma(dy, dy, dx * dx)); both agree bit for bit wherever every step is exact (integer and half-integer lattices), which is
where the bit-equality tests run.  Elsewhere the tests use float64 truths with tie tolerances, or the FPS certificate.

FPS: sel[0] = start; cur = init for finite points, -inf for points with a non-finite coordinate; step s: cur = min(cur, d2(., sel[s-1]))
with NaN distances ignored, sel[s] = the lowest index of max cur.
kNN: candidates of the same example with d2 < 1e10, ordered by (d2, index), the first k; empty slots hold -1 (d2 +inf).
"""
import numpy as np

KNN_NONE = 1e10


def lattice(n, dims=3, seed=None, scale=1.0, offset=0.0):
    """The n^dims integer lattice as float32 [n^dims, 3] (unused axes 0), optionally permuted with `seed`."""
    g = np.stack(np.meshgrid(*[np.arange(n)] * dims, indexing="ij"), -1).reshape(-1, dims).astype(np.float64)
    x = np.zeros((g.shape[0], 3))
    x[:, :dims] = g * scale + offset
    if seed is not None:
        x = x[np.random.default_rng(seed).permutation(x.shape[0])]
    return x.astype(np.float32)


def d2_f32(q, P):
    """float32 squared distances of the point q [3] to the points P [N, 3] (float32 differences, exact where the lattice is)."""
    d = (np.asarray(P, np.float32) - np.asarray(q, np.float32)[None, :]).astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)


def fps_restate(xyz, n_samples, start, init_d2):
    """igs_fps for one example: indices into xyz in selection order."""
    xyz = np.asarray(xyz, np.float32)
    fin = np.isfinite(xyz).all(1)
    cur = np.where(fin, np.float32(init_d2), np.float32(-np.inf)).astype(np.float32)
    sel = [int(start)]
    for _ in range(1, n_samples):
        cur = np.fmin(cur, d2_f32(xyz[sel[-1]], xyz))
        sel.append(int(np.argmax(cur)))                   # the first maximum: ties to the lowest index
    return np.array(sel, dtype=np.int64)


def fps_f64(xyz, n_samples, start):
    """An independent float64 vanilla FPS (finite points only): an explicit loop, ties to the lowest index."""
    x = np.asarray(xyz, np.float64)
    n = x.shape[0]
    best = [float("inf")] * n
    sel = [int(start)]
    for _ in range(1, n_samples):
        p = x[sel[-1]]
        far, arg = -1.0, -1
        for i in range(n):
            d = (x[i, 0] - p[0]) ** 2 + (x[i, 1] - p[1]) ** 2 + (x[i, 2] - p[2]) ** 2
            if d < best[i]:
                best[i] = d
            if best[i] > far:
                far, arg = best[i], i
        sel.append(arg)
    return np.array(sel, dtype=np.int64)


def fps_certificate(xyz, sel, rel=1e-6):
    """Checks a sampling against the definition of FPS in float64: no index repeats and every pick's distance to the earlier picks is
    >= (1 - rel) times the largest such distance over all points.  Holds for any correct FPS, whatever the rounding.  xyz: a torch
    tensor or numpy array (the work runs on its device)."""
    import torch
    x = torch.as_tensor(xyz).double()
    s = torch.as_tensor(sel, device=x.device).long()
    assert s.unique().numel() == s.numel(), "an index repeats"
    cur = torch.full((x.shape[0],), float("inf"), dtype=torch.float64, device=x.device)
    ratios = []
    for i in range(1, s.numel()):
        cur = torch.minimum(cur, ((x - x[s[i - 1]]) ** 2).sum(1))
        m = cur.max()
        ratios.append(torch.where(m > 0, cur[s[i]] / m, torch.ones_like(m)))
    worst = float(torch.stack(ratios).min()) if ratios else 1.0
    assert worst >= 1.0 - rel, f"a pick is {worst} of the farthest distance"
    return worst


def knn_restate(x, y, k, ptr_x=None, ptr_y=None):
    """igs_knn_query: (idx [Ny, k] int64, -1 padded; d2 [Ny, k] float32, +inf padded)."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    ptr_x = [0, x.shape[0]] if ptr_x is None else list(ptr_x)
    ptr_y = [0, y.shape[0]] if ptr_y is None else list(ptr_y)
    idx = np.full((y.shape[0], k), -1, np.int64)
    dd = np.full((y.shape[0], k), np.inf, np.float32)
    for b in range(len(ptr_y) - 1):
        xs = x[ptr_x[b]:ptr_x[b + 1]]
        for j in range(ptr_y[b], ptr_y[b + 1]):
            d = d2_f32(y[j], xs)
            cand = np.nonzero(d < KNN_NONE)[0]
            order = cand[np.lexsort((cand, d[cand]))][:k]
            idx[j, :order.size] = order + ptr_x[b]
            dd[j, :order.size] = d[order]
    return idx, dd


def knn_f64(x, y, k, ptr_x=None, ptr_y=None):
    """float64 truth: (idx [Ny, k], d2 [Ny, k + 1]: the k + 1 smallest float64 distances, for the tie tolerance at the k-th)."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    ptr_x = [0, x.shape[0]] if ptr_x is None else list(ptr_x)
    ptr_y = [0, y.shape[0]] if ptr_y is None else list(ptr_y)
    idx = np.full((y.shape[0], k), -1, np.int64)
    dd = np.full((y.shape[0], k + 1), np.inf)
    for b in range(len(ptr_y) - 1):
        xs = x[ptr_x[b]:ptr_x[b + 1]]
        for j in range(ptr_y[b], ptr_y[b + 1]):
            d = ((xs - y[j]) ** 2).sum(1)
            o = np.lexsort((np.arange(d.size), d))[:k + 1]
            idx[j, :min(k, o.size)] = o[:k] + ptr_x[b]
            dd[j, :o.size] = d[o]
    return idx, dd


def select_restate(xyz_list, bbox):
    """select_points_bbox per example: the ascending indices with lo <= p <= hi on every axis (NaN: outside)."""
    out = []
    for x, b in zip(xyz_list, bbox):
        x = np.asarray(x, np.float32)
        b = np.asarray(b, np.float32).reshape(2, 3)
        with np.errstate(invalid="ignore"):
            m = ((x >= b[0]) & (x <= b[1])).all(1)
        out.append(np.nonzero(m)[0].astype(np.int64))
    return out
