"""The anchor graph on the GPU (anchors.hip: igs_bbox_select, igs_fps, igs_knn_query) through the torch_cluster and fpsample drop-ins
and igs_amd.anchors, against tests/anchors_restatement.py: lattice bit-equality, float64 truths with tie tolerances, the FPS
certificate, batching, float batch ids, empty inputs, strided input on a side stream, determinism, and get_mask_fpsample restated
literally through the two drop-ins."""
import math

import numpy as np
import pytest
import torch

import anchors_restatement as AR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _cuda(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def _knn_native(x, y, k, ptr_x=None, ptr_y=None, weight_scale=None):
    from igs_amd import anchors as A
    px = torch.tensor([0, x.shape[0]] if ptr_x is None else list(ptr_x), dtype=torch.int32, device=DEV)
    py = torch.tensor([0, y.shape[0]] if ptr_y is None else list(ptr_y), dtype=torch.int32, device=DEV)
    idx, d2, w = A.knn_native(_cuda(x), _cuda(y), k, px, py, with_d2=True, weight_scale=weight_scale)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy(), (None if w is None else w.cpu().numpy())


def _fps_native(x, n_samples, start, init_d2):
    from igs_amd import anchors as A
    i32 = dict(dtype=torch.int32, device=DEV)
    out = A.fps_native(_cuda(x), torch.tensor([0, x.shape[0]], **i32), torch.tensor([start], **i32), torch.tensor([0, n_samples], **i32),
                       n_samples, x.shape[0], init_d2)
    return out.cpu().numpy()


def _clustered(n, seed):
    g = np.random.default_rng(seed)
    c = g.normal(size=(10, 3)) * 3
    w = g.uniform(0.01, 0.3, 10)
    k = g.integers(0, 10, n)
    return (c[k] + g.normal(size=(n, 3)) * w[k, None]).astype(np.float32)


# ---------------------------------------------------------------- knn
@pytest.mark.parametrize("k", [1, 8, 16, 100])
def test_knn_lattice_bit_equal(k):
    x = AR.lattice(6, seed=k)                                          # 216 points, ties everywhere
    y = np.concatenate([AR.lattice(5, seed=k + 1, offset=0.5), AR.lattice(3, seed=k + 2, scale=2.0)])
    idx, d2, _ = _knn_native(x, y, k)
    ridx, rd2 = AR.knn_restate(x, y, k)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(d2, rd2)


def _check_vs_f64(x, y, k, idx, ptr_x=None, ptr_y=None):
    tidx, td = AR.knn_f64(x, y, k, ptr_x, ptr_y)
    bad = np.nonzero((idx != tidx).any(1))[0]
    for j in bad:
        # allowed only where the k-th and (k+1)-th float64 distances lie within 4 ulp (of float32)
        kth, nxt = td[j, k - 1], td[j, k]
        assert nxt - kth <= 4 * np.spacing(np.float32(kth)), (j, idx[j], tidx[j])
        xs = np.asarray(x, np.float64)
        got = np.sort(((xs[idx[j]] - y[j]) ** 2).sum(1))
        np.testing.assert_allclose(got, td[j, :k], rtol=1e-5, atol=1e-12)
    return bad.size


@pytest.mark.parametrize("cloud", ["uniform", "clustered"])
def test_knn_float_clouds_match_f64(cloud):
    g = np.random.default_rng(3)
    x = g.random((3000, 3), dtype=np.float32) if cloud == "uniform" else _clustered(3000, 4)
    y = g.random((2000, 3), dtype=np.float32) if cloud == "uniform" else _clustered(2000, 5)
    idx, d2, _ = _knn_native(x, y, 8)
    assert _check_vs_f64(x, y, 8, idx) <= 4


def test_knn_batched_unequal_sizes_and_dropin():
    from torch_cluster import knn
    g = np.random.default_rng(6)
    nx, ny = [50, 5, 300], [40, 30, 7]                                  # the middle example has fewer than k = 8 points
    x = (g.integers(0, 20, (sum(nx), 3))).astype(np.float32)
    y = (g.integers(0, 20, (sum(ny), 3))).astype(np.float32)
    px, py = np.concatenate([[0], np.cumsum(nx)]), np.concatenate([[0], np.cumsum(ny)])
    idx, d2, _ = _knn_native(x, y, 8, px, py)
    ridx, rd2 = AR.knn_restate(x, y, 8, px, py)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(d2, rd2)
    bx = torch.repeat_interleave(torch.arange(3), torch.tensor(nx)).to(DEV)
    by = torch.repeat_interleave(torch.arange(3), torch.tensor(ny)).float().to(DEV)      # float batch_y, as gs.py passes
    e = knn(_cuda(x), _cuda(y), 8, bx, by).cpu().numpy()
    m = ridx >= 0
    rows = np.repeat(np.arange(y.shape[0])[:, None], 8, 1)
    np.testing.assert_array_equal(e, np.stack([rows[m], ridx[m]]))
    assert e.shape[1] == sum(ny) * 8 - 30 * 3                          # 30 queries of the 5-point example keep 5 of 8


def test_knn_empty_inputs():
    from torch_cluster import knn
    z = torch.zeros(0, 3, device=DEV)
    p = torch.rand(10, 3, device=DEV)
    for a, b in ((z, p), (p, z), (z, z)):
        e = knn(a, b, 4)
        assert e.shape == (2, 0) and e.dtype == torch.int64


def test_knn_strided_input_on_side_stream():
    from torch_cluster import knn
    g = torch.Generator().manual_seed(7)
    big = torch.rand(400, 6, generator=g).to(DEV)
    x, y = big[:, ::2], big[:300, 1::2]                                 # non-contiguous views
    ref = knn(x.contiguous(), y.contiguous(), 8)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = knn(x, y, 8)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_knn_igs_size_matches_torch_brute_force():
    g = torch.Generator().manual_seed(8)
    anchors = torch.rand(8192, 3, generator=g).to(DEV)
    pts = torch.rand(200000, 3, generator=g).to(DEV)
    from igs_amd import anchors as A
    i32 = dict(dtype=torch.int32, device=DEV)
    idx, d2, _ = A.knn_native(anchors, pts, 8, torch.tensor([0, 8192], **i32), torch.tensor([0, 200000], **i32), with_d2=True)
    torch.cuda.synchronize()
    bad = 0
    for a in range(0, pts.shape[0], 4096):
        q = pts[a:a + 4096].double()
        d = ((q[:, None, :] - anchors.double()[None]) ** 2).sum(-1)
        tv, ti = torch.topk(d, 9, dim=1, largest=False)
        differ = (torch.sort(idx[a:a + 4096], 1).values != torch.sort(ti[:, :8], 1).values).any(1)
        tied = (tv[:, 8] - tv[:, 7]) <= 4 * tv[:, 7] * 2.0 ** -23         # k-th and (k+1)-th within 4 ulp
        bad += int((differ & ~tied).sum())
        assert torch.allclose(d2[a:a + 4096].double(), tv[:, :8], rtol=1e-6, atol=1e-12)
    assert bad == 0


def test_knn_weights_softmax():
    g = np.random.default_rng(9)
    x = g.random((500, 3), dtype=np.float32)
    y = g.random((300, 3), dtype=np.float32)
    idx, d2, w = _knn_native(x, y, 8, weight_scale=10.0)
    ref = torch.softmax(-10 * torch.from_numpy(d2).double().sqrt(), -1).numpy()
    np.testing.assert_allclose(w, ref, rtol=1e-5, atol=1e-7)


# ---------------------------------------------------------------- fps
@pytest.mark.parametrize("start", [0, 17, 300])
@pytest.mark.parametrize("init", [5e4, math.inf])
def test_fps_lattice_bit_equal(start, init):
    x = AR.lattice(8, seed=start + 1)                                  # 512 points: every step is full of ties
    got = _fps_native(x, 200, start, init)
    np.testing.assert_array_equal(got, AR.fps_restate(x, 200, start, init))


def test_fps_large_lattice_bit_equal():
    x = AR.lattice(40, seed=5, scale=0.5)                              # 64000 points: 1000 leaves over the 16 waves
    got = _fps_native(x, 500, 1234, math.inf)
    np.testing.assert_array_equal(got, AR.fps_restate(x, 500, 1234, math.inf))


@pytest.mark.parametrize("cloud", ["uniform", "clustered"])
def test_fps_float_cloud_certificate(cloud):
    g = np.random.default_rng(10)
    x = g.random((20000, 3), dtype=np.float32) if cloud == "uniform" else _clustered(20000, 11)
    sel = _fps_native(x, 1000, 3, math.inf)
    AR.fps_certificate(_cuda(x), sel)


def test_fps_non_finite_points_never_selected():
    g = np.random.default_rng(12)
    x = g.random((3000, 3), dtype=np.float32)
    bad = g.choice(3000, 50, replace=False)
    x[bad[:25], 0] = np.nan
    x[bad[25:], 2] = np.inf
    sel = _fps_native(x, 500, int(np.setdiff1d(np.arange(3000), bad)[0]), math.inf)
    assert not np.isin(sel, bad).any()
    fin = np.setdiff1d(np.arange(3000), bad)
    AR.fps_certificate(_cuda(x[fin]), np.searchsorted(fin, sel))


def test_fps_sear_steak_size_certificate():
    from igs_amd import scenes
    raw, _, _ = scenes.sear_steak_like_scene(P=200000)
    x = raw["xyz"].float().to(DEV)
    sel = _fps_native(x.cpu().numpy(), 8192, 0, math.inf)
    AR.fps_certificate(x, sel)


def test_torch_cluster_fps_counts_starts_and_seed():
    from torch_cluster import fps
    g = torch.Generator().manual_seed(13)
    n = [100, 37, 1, 250]
    src = torch.rand(sum(n), 3, generator=g).to(DEV)
    batch = torch.repeat_interleave(torch.arange(4), torch.tensor(n)).to(DEV)
    ptr = np.concatenate([[0], np.cumsum(n)])
    for ratio in (0.5, 0.1, 0.33, 1.0):
        out = fps(src, batch, ratio=ratio, random_start=False).cpu().numpy()
        want = [int(math.ceil(np.float32(c) * np.float32(ratio))) for c in n]
        assert out.size == sum(want)
        o = np.concatenate([[0], np.cumsum(want)])
        for b in range(4):
            seg = out[o[b]:o[b + 1]]
            assert seg[0] == ptr[b] and ((seg >= ptr[b]) & (seg < ptr[b + 1])).all() and np.unique(seg).size == seg.size
    torch.manual_seed(5)
    a = fps(src, batch, ratio=0.25)
    torch.manual_seed(5)
    b = fps(src, batch, ratio=0.25)
    assert torch.equal(a, b)
    torch.manual_seed(5)
    st = (torch.rand(4, device=DEV) * torch.tensor(n, device=DEV).float()).long().cpu().numpy()
    firsts = a.cpu().numpy()[np.concatenate([[0], np.cumsum([math.ceil(c * 0.25) for c in n])[:-1]])]
    np.testing.assert_array_equal(firsts, ptr[:-1] + st)


def test_fpsample_dropin_equals_native():
    import fpsample
    g = np.random.default_rng(14)
    x = g.random((5000, 3), dtype=np.float32)
    out = fpsample.bucket_fps_kdline_sampling(x, 256, h=5, start_idx=42)
    assert out.dtype == np.int64 and out.shape == (256,)
    np.testing.assert_array_equal(out, _fps_native(x, 256, 42, math.inf))
    np.random.seed(3)
    a = fpsample.bucket_fps_kdline_sampling(x, 64, h=5)
    np.random.seed(3)
    assert a[0] == np.random.randint(5000)


def test_runs_are_bit_identical():
    g = np.random.default_rng(15)
    x = _clustered(50000, 16)
    y = g.random((20000, 3), dtype=np.float32)
    a = _fps_native(x, 2048, 7, math.inf), _knn_native(x, y, 8, weight_scale=10.0)
    b = _fps_native(x, 2048, 7, math.inf), _knn_native(x, y, 8, weight_scale=10.0)
    np.testing.assert_array_equal(a[0], b[0])
    for u, v in zip(a[1], b[1]):
        np.testing.assert_array_equal(u, v)


# ---------------------------------------------------------------- anchor_graph
def _get_mask_fpsample_literal(gs_xyz, bbox, anchor_size, starts):
    """igs/models/gs.py:966-1011 with the reference's own calls, through the two drop-ins (start_idx added to fix the draws)."""
    import fpsample
    from torch_cluster import knn
    masks, anchor_points, points, batch_y, anchor_idx = [], [], [], [], []
    batchsize = len(gs_xyz)
    for idx, xyz in enumerate(gs_xyz):
        b = bbox[idx][None]
        p = xyz[None]
        index_inbbox = torch.where(
            (p[:, :, 0] >= b[:, 0, 0, None]) & (p[:, :, 0] <= b[:, 1, 0, None]) &
            (p[:, :, 1] >= b[:, 0, 1, None]) & (p[:, :, 1] <= b[:, 1, 1, None]) &
            (p[:, :, 2] >= b[:, 0, 2, None]) & (p[:, :, 2] <= b[:, 1, 2, None]))[1]
        masks.append(index_inbbox)
        pc = xyz[index_inbbox]
        s = fpsample.bucket_fps_kdline_sampling(pc.detach().cpu().numpy(), anchor_size, h=5, start_idx=starts[idx])
        anchor_points.append(pc[torch.from_numpy(s.astype(np.int64))])
        points.append(pc)
        batch_y.append(torch.zeros(pc.shape[0]) + idx)
        anchor_idx.append(s.astype(int))
    points = torch.cat(points, dim=0)
    batch_y = torch.cat(batch_y, dim=0).to(points.device)
    anchor_points = torch.stack(anchor_points, dim=0)
    anchor_flatten = anchor_points.reshape(-1, 3)
    batch_x = torch.repeat_interleave(torch.arange(batchsize).to(DEV), anchor_flatten.shape[0] // batchsize)
    row, col = knn(anchor_flatten, points, 8, batch_x, batch_y)
    dist = torch.linalg.vector_norm(anchor_flatten[col] - points[row], ord=2, dim=-1)
    weights = torch.softmax(-10 * dist.view(-1, 8), dim=-1).unsqueeze(-1)
    return anchor_points, masks, weights, (row, col, batch_x, batch_y), anchor_idx


def test_anchor_graph_matches_literal_get_mask_fpsample():
    from igs_amd.anchors import anchor_graph
    g = torch.Generator().manual_seed(17)
    xyz = [(torch.rand(30000, 3, generator=g) * 4 - 2).to(DEV), (torch.randn(24000, 3, generator=g)).to(DEV)]
    bbox = torch.tensor([[[-1.5, -1.0, -1.8], [1.2, 1.9, 1.0]], [[-1.0, -1.2, -0.9], [1.1, 0.8, 1.3]]], device=DEV)
    starts = [11, 4000]
    A = 1024
    got = anchor_graph(xyz, bbox, anchor_size=A, k=8, start_idx=starts)
    ref = _get_mask_fpsample_literal(xyz, bbox, A, starts)
    assert torch.equal(got[0], ref[0])
    for m, r in zip(got[1], ref[1]):
        assert m.dtype == torch.int64 and torch.equal(m, r)
    assert got[2].shape == ref[2].shape
    torch.testing.assert_close(got[2], ref[2], rtol=1e-5, atol=1e-6)
    for a, r in zip(got[3], ref[3]):
        assert a.dtype == r.dtype and torch.equal(a, r)
    for a, r in zip(got[4], ref[4]):
        np.testing.assert_array_equal(a.cpu().numpy(), r)


def test_anchor_graph_too_few_points_raises():
    from igs_amd.anchors import anchor_graph
    x = torch.rand(500, 3, device=DEV)
    bbox = torch.tensor([[[0.0, 0.0, 0.0], [0.5, 0.5, 0.5]]], device=DEV)
    with pytest.raises(ValueError, match="fewer than anchor_size"):
        anchor_graph([x], bbox, anchor_size=256)
