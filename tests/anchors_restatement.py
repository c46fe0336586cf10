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


# ---------------------------------------------------------------- launch geometry, restated from anchors.hip (source lines cited)
FPS_WAVES = 16                 # anchors.hip:20
FPS_MAX_SLOTS = 4              # anchors.hip:21
KNNQ_THREADS = 256             # anchors.hip:22  queries per kNN workgroup
KNNQ_TILE = 2048               # anchors.hip:23  x points per LDS tile
KNN_SLOT_CLASSES = (8, 16, 32, 100)       # anchors.hip:512-515  launch_knn_query's instantiations
SELECT_BLOCK = 256             # anchors.hip:139  points per select workgroup (one block sum each)
SCAN_THREADS = 1024            # radix_sort.hip:19-25  the single-block scan: ceil(n / 1024) entries per thread


def fps_geometry(max_n):
    """anchors.hip:152-160 fps_geometry: (LS, R) = (rows per leaf, leaf records per lane) for a launch sized by max_n."""
    m = 1
    while max_n > FPS_WAVES * 64 * FPS_MAX_SLOTS * 64 * m:
        m *= 2
    leaves = (max_n + 64 * m - 1) // (64 * m)
    r = 1
    while FPS_WAVES * 64 * r < leaves:
        r *= 2
    return 64 * m, r


def fps_example_bits(B):
    """anchors.hip:406-408: bits of the example-keyed sort round (none for B = 1); ceil(bits / 8) radix passes."""
    if B <= 1:
        return 0
    bits = 0
    while (1 << bits) < B:
        bits += 1
    return bits


def knn_slot_class(k):
    """anchors.hip:512-515: the register slots K of the instantiation that serves k."""
    return next(c for c in KNN_SLOT_CLASSES if k <= c)


def knn_straddling_workgroups(ptr_y):
    """Per kNN workgroup (256 consecutive queries, anchors.hip:439-445): True where its first and last query lie in different
    examples -- the workgroups the masked instantiation serves."""
    ptr_y = np.asarray(ptr_y)
    ny = int(ptr_y[-1])
    out = []
    for first in range(0, ny, KNNQ_THREADS):
        last = min(first + KNNQ_THREADS, ny) - 1
        out.append(bool(np.searchsorted(ptr_y, first, "right") != np.searchsorted(ptr_y, last, "right")))
    return out


def select_scan_per_thread(n):
    """Entries per thread of the single-block scan over the select's block sums (anchors.hip:139-141, radix_sort.hip:25)."""
    nb = (n + SELECT_BLOCK - 1) // SELECT_BLOCK
    return (nb + SCAN_THREADS - 1) // SCAN_THREADS


# ---------------------------------------------------------------- case builders of tests/test_gpu_anchors_edges.py
def with_non_finite(x, rows, what=(np.nan, np.inf, -np.inf)):
    """A copy of x whose `rows` carry, in turn, a NaN, +inf, -inf in the axis row % 3."""
    x = np.array(x, np.float32)
    for j, r in enumerate(rows):
        x[r, r % 3] = what[j % len(what)]
    return x


def select_case(n, seed=0):
    """(xyz [n, 3], box [2, 3]): the first n rows of a permuted half-integer lattice of side s (coordinates 0, 0.5, ...) and the box
    [0.5, (s - 2) / 2]^3, so the lattice's second and second-to-last layers lie exactly on the faces (kept: lo <= p <= hi) and the
    outermost layers half a step outside; about 1 % of the rows (three at least from 63 rows on) carry a NaN, +inf or -inf."""
    s = max(4, int(np.ceil(n ** (1.0 / 3.0) - 1e-9)))
    while s ** 3 < n:
        s += 1
    x = lattice(s, seed=seed, scale=0.5)[:n]
    g = np.random.default_rng(seed + 1)
    nbad = 0 if n < 63 else max(3, n // 100)
    x = with_non_finite(x, g.choice(n, nbad, replace=False))
    box = np.array([[0.5, 0.5, 0.5], [(s - 2) * 0.5] * 3], np.float32)
    return x, box


SELECT_BATCH_SIZES = (100, 0, 37, 1, 300)


def select_batch_case(seed=0):
    """(list of xyz, boxes [5, 2, 3]) for SELECT_BATCH_SIZES: example 0 all inside its box, 1 empty, 2 and 4 cut by face boxes (with
    non-finite rows), 3 (a single point) all outside."""
    xs, boxes = [], []
    for b, n in enumerate(SELECT_BATCH_SIZES):
        x, box = select_case(max(n, 1), seed=seed + 10 * b)
        x = x[:n]
        if b == 0:
            x = lattice(5, seed=seed, scale=0.5)[:n]
            box = np.array([[-1, -1, -1], [100, 100, 100]], np.float32)
        if b == 3:
            box = np.array([[50, 50, 50], [60, 60, 60]], np.float32)
        xs.append(x)
        boxes.append(box)
    return xs, np.stack(boxes)


def clustered(n, seed):
    """A float cloud of ten Gaussian clusters of unequal widths."""
    g = np.random.default_rng(seed)
    c = g.normal(size=(10, 3)) * 3
    w = g.uniform(0.01, 0.3, 10)
    k = g.integers(0, 10, n)
    return (c[k] + g.normal(size=(n, 3)) * w[k, None]).astype(np.float32)


# name: (lattice side, samples, start, the (LS, R) class the case is there for)
FPS_CLASS_CASES = {"R2": (41, 200, 40000, (64, 2)), "R4": (51, 200, 777, (64, 4)),
                   "LS128": (65, 150, 123456, (128, 4)), "LS256": (81, 100, 500000, (256, 4))}
FPS_CERT_R2 = (100000, 500)                # points, samples of the clustered float cloud at R = 2
FPS_BATCH_SIDES = (8, 4, 10, 3)            # 512, 64, 1000 and 27 points
FPS_BATCH_SAMPLES = (200, 64, 300, 27)     # examples 1 and 3 are sampled completely
FPS_BATCH_STARTS = (5, 63, 999, 0)
FPS_MANY = (300, 5, 10)                    # examples, lattice side, samples each


def fps_batch_case():
    """The four lattices of FPS_BATCH_SIDES, the 1000-point one with five non-finite rows (none of them its start)."""
    xs = [lattice(s, seed=20 + b) for b, s in enumerate(FPS_BATCH_SIDES)]
    xs[2] = with_non_finite(xs[2], [3, 100, 501, 777, 998])
    return xs


def knn_masked_case(seed=0):
    """Integer coordinates in [0, 12): (x, y, ptr_x, ptr_y) with nx = [2049, 40, 300] (example 0 spans two LDS tiles, example 1 has
    fewer than k = 100 points) and ny = [250, 20, 330] (workgroups 0 and 1 straddle examples, workgroup 2 does not)."""
    g = np.random.default_rng(seed)
    nx, ny = [2049, 40, 300], [250, 20, 330]
    x = g.integers(0, 12, (sum(nx), 3)).astype(np.float32)
    y = g.integers(0, 12, (sum(ny), 3)).astype(np.float32)
    return x, y, np.concatenate([[0], np.cumsum(nx)]), np.concatenate([[0], np.cumsum(ny)])


def knn_cut_case():
    """(x, y): from the query at the origin (99 999, 0, 0) is kept and (100 000, 0, 0), at d2 = 1e10 exactly, dropped; rows of x carry
    NaN and +-inf; query 1 is NaN (no neighbour at all), query 2 an ordinary point."""
    x = np.array([[99999, 0, 0], [100000, 0, 0], [np.nan, 0, 0], [1, 2, 2], [0, np.inf, 0], [0, 3, 4], [-np.inf, 1, 1], [0, 0, np.nan],
                  [2, 0, 0], [0, -2, 0]], np.float32)
    y = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 1, 1]], np.float32)
    return x, y


def knn_weights_f64(d2, idx, scale):
    """softmax(-scale * sqrt(d2)) in float64 over the filled slots (idx >= 0) of every row; 0 in the empty ones and in rows without a
    neighbour."""
    d = np.sqrt(np.asarray(d2, np.float64))
    has = np.asarray(idx) >= 0
    z = np.where(has, -scale * np.where(has, d, 0.0), -np.inf)
    m = np.where(has.any(1, keepdims=True), z.max(1, keepdims=True, initial=-np.inf), 0.0)
    e = np.where(has, np.exp(z - m), 0.0)
    s = e.sum(1, keepdims=True)
    return np.where(has, e / np.where(s > 0, s, 1.0), 0.0)
