"""The anchor-graph kernels (anchors.hip: igs_bbox_select, igs_fps, igs_knn_query) at the launch branches tests/test_gpu_anchors.py
does not reach: every fps_kernel<R> and leaf width, batched FPS sequences, the two-pass example sort, the documented -1 / clamp /
truncation outcomes, knnq_kernel<32, *> and the masked instantiations above k = 8, the LDS tile and workgroup edges, the d2 < 1e10
cut, non-finite rows, and the in-box select on box faces, across example boundaries and past 1024 block sums.

Every case has integer or half-integer coordinates (all distances exact in float32) and is compared bit for bit with
tests/anchors_restatement.py -- no tolerance, no excluded row -- except the clustered float cloud, which is held to the FPS
certificate, and the kNN weights, held to the float64 softmax with test_gpu_anchors.py's rule (rtol 1e-5, atol 1e-7).
tests/test_anchors_host.py asserts without a GPU that each size below lands in the class its test names.
"""
import functools
import math

import numpy as np
import pytest
import torch

import anchors_restatement as AR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BAND = 64                      # sentinel elements around every C-ABI output
I64_SENTINEL = -777
F32_SENTINEL = -777.0


def _cuda(a):
    return torch.tensor(np.asarray(a)).to(DEV)                     # (a copy: the shared cases are read-only)


def _i32(a):
    return torch.tensor([int(v) for v in a], dtype=torch.int32, device=DEV)


def _ptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _lib():
    from igs_amd import _cabi
    return _cabi.lib()


def _ok(rc):
    from igs_amd import _cabi
    assert rc == 0, _cabi.last_error()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _banded(n, dtype, fill):
    """(whole buffer, the n-element view BAND elements inside it), all `fill`."""
    big = torch.full((n + 2 * BAND,), fill, dtype=dtype, device=DEV)
    return big, big[BAND:BAND + n]


def _bands_intact(big, n, fill):
    return bool((big[:BAND] == fill).all() and (big[BAND + n:] == fill).all())


# ---------------------------------------------------------------- igs_bbox_select
def _select_native(xs, boxes):
    from igs_amd import anchors as A
    xyz = np.concatenate(xs) if len(xs) > 1 else xs[0]
    oxyz, oidx, cnt = A.bbox_select(_cuda(xyz), _i32(_ptr([len(x) for x in xs])), _cuda(np.asarray(boxes, np.float32).reshape(-1, 2, 3)))
    torch.cuda.synchronize()
    return oxyz.cpu().numpy(), oidx.cpu().numpy(), cnt.cpu().numpy()


def _check_select(xs, boxes, got):
    oxyz, oidx, cnt = got
    want = AR.select_restate(xs, boxes)
    np.testing.assert_array_equal(cnt, [w.size for w in want])
    total = int(cnt.sum())
    np.testing.assert_array_equal(oidx[:total], np.concatenate(want))
    kept = np.concatenate([x[w] for x, w in zip(xs, want)]).astype(np.float32)
    np.testing.assert_array_equal(oxyz[:total].view(np.uint32), kept.view(np.uint32))
    return total


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025, 300000])
def test_select_sizes_faces_and_non_finite(n):
    """Points exactly on lo and hi are kept, NaN / +-inf rows dropped; 300 000 points give 1172 block sums (two per scan thread)."""
    x, box = AR.select_case(n, seed=n)
    total = _check_select([x], [box], _select_native([x], [box]))
    if n >= 63:
        on_face = ((x == box[0]) | (x == box[1])).any(1) & np.isfinite(x).all(1)
        assert on_face.any() and 0 < total < n


def test_select_degenerate_and_inverted_box():
    x, box = AR.select_case(1025, seed=3)
    flat = box.copy()
    flat[:, 2] = 1.0                                   # lo == hi on z: the plane z = 1 exactly
    assert _check_select([x], [flat], _select_native([x], [flat])) > 0
    inv = box[::-1].copy()                             # lo > hi: nothing
    assert _check_select([x], [inv], _select_native([x], [inv])) == 0


def test_select_batched_boundaries_inside_waves():
    """Sizes [100, 0, 37, 1, 300]: the boundaries at 100, 137 and 138 lie inside waves of workgroup 0 (the per-lane atomic path), one
    example is empty; indices are relative to the example and example order is kept."""
    xs, boxes = AR.select_batch_case()
    got = _select_native(xs, boxes)
    _check_select(xs, boxes, got)
    assert got[2][0] == 100 and got[2][1] == 0 and got[2][3] == 0 and 0 < got[2][2] < 37 and 0 < got[2][4] < 300


def test_select_cabi_writes_nothing_past_the_total():
    """Outputs and scratch inside sentinel bands; the scratch is exactly igs_bbox_select_scratch_bytes(N)."""
    L = _lib()
    n = 1025
    x, box = AR.select_case(n, seed=5)
    want = AR.select_restate([x], [box])[0]
    xd, bd, pd = _cuda(x), _cuda(box), _i32([0, n])
    sbytes = L.igs_bbox_select_scratch_bytes(n)
    assert sbytes > 0
    sbig, _ = _banded(sbytes, torch.uint8, 0xA5)
    xbig, oxyz = _banded(3 * n, torch.float32, F32_SENTINEL)
    ibig, oidx = _banded(n, torch.int64, I64_SENTINEL)
    cbig, cnt = _banded(1, torch.int32, I64_SENTINEL)
    _ok(L.igs_bbox_select(_stream(), 1, n, xd.data_ptr(), pd.data_ptr(), bd.data_ptr(), sbig.data_ptr() + BAND, oxyz.data_ptr(),
                          oidx.data_ptr(), cnt.data_ptr()))
    torch.cuda.synchronize()
    t = want.size
    assert int(cnt[0]) == t and 0 < t < n
    np.testing.assert_array_equal(oidx[:t].cpu().numpy(), want)
    np.testing.assert_array_equal(oxyz[:3 * t].cpu().numpy().reshape(-1, 3).view(np.uint32), x[want].view(np.uint32))
    assert (oidx[t:] == I64_SENTINEL).all() and (oxyz[3 * t:] == F32_SENTINEL).all(), "an entry at or past the total was written"
    assert _bands_intact(sbig, sbytes, 0xA5) and _bands_intact(xbig, 3 * n, F32_SENTINEL)
    assert _bands_intact(ibig, n, I64_SENTINEL) and _bands_intact(cbig, 1, I64_SENTINEL)


# ---------------------------------------------------------------- igs_fps
def _fps_native(xs, samples, starts, init_d2=math.inf, max_n=None):
    """One launch over the examples xs; returns the per-example segments (global indices)."""
    from igs_amd import anchors as A
    xyz = np.concatenate(xs) if len(xs) > 1 else xs[0]
    optr = _ptr(samples)
    out = A.fps_native(_cuda(xyz), _i32(_ptr([len(x) for x in xs])), _i32(starts), _i32(optr), int(optr[-1]),
                       max(len(x) for x in xs) if max_n is None else max_n, init_d2)
    out = out.cpu().numpy()
    return [out[optr[b]:optr[b + 1]] for b in range(len(xs))]


@functools.lru_cache(maxsize=None)
def _class_case(name):
    """(points, the restatement's sequence) of one FPS_CLASS_CASES entry: built once, shared, never changed."""
    side, samples, start, _ = AR.FPS_CLASS_CASES[name]
    x = AR.lattice(side, seed=side)
    ref = AR.fps_restate(x, samples, start, math.inf)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


@pytest.mark.parametrize("name", list(AR.FPS_CLASS_CASES))
def test_fps_geometry_classes_bit_equal(name):
    """fps_kernel<2>, fps_kernel<4>, and leaves of 128 and 256 rows: the restatement's sequence, every pick full of ties."""
    _, samples, start, _ = AR.FPS_CLASS_CASES[name]
    x, ref = _class_case(name)
    (got,) = _fps_native([x], [samples], [start])
    np.testing.assert_array_equal(got, ref)


def test_fps_certificate_at_two_slots():
    n, samples = AR.FPS_CERT_R2
    x = AR.clustered(n, 31)
    (sel,) = _fps_native([x], [samples], [17])
    worst = AR.fps_certificate(_cuda(x), sel, rel=1e-6)
    print(f"fps certificate, {n} clustered points at R = 2: worst pick at {worst:.9f} of the farthest distance")


def test_fps_batched_sequences_bit_equal():
    """Four lattices in one launch, two of them sampled completely, starts at the first and last rows, non-finite rows in one."""
    xs = AR.fps_batch_case()
    got = _fps_native(xs, AR.FPS_BATCH_SAMPLES, AR.FPS_BATCH_STARTS)
    ptr = _ptr([len(x) for x in xs])
    for b, x in enumerate(xs):
        ref = AR.fps_restate(x, AR.FPS_BATCH_SAMPLES[b], AR.FPS_BATCH_STARTS[b], math.inf)
        np.testing.assert_array_equal(got[b], ref + ptr[b], err_msg=f"example {b}")
        if AR.FPS_BATCH_SAMPLES[b] == len(x):
            np.testing.assert_array_equal(np.sort(got[b]), np.arange(ptr[b], ptr[b + 1]))


def test_fps_mixed_geometry_small_example_in_a_wide_leaf():
    """The 65^3 lattice (leaves of 128 rows) beside a 100-point example, which gets one padded 128-row leaf."""
    side, samples, start, _ = AR.FPS_CLASS_CASES["LS128"]
    x, ref = _class_case("LS128")
    small = AR.lattice(5, seed=9)[:100]
    got = _fps_native([x, small], [samples, 60], [start, 99])
    np.testing.assert_array_equal(got[0], ref)
    np.testing.assert_array_equal(got[1], AR.fps_restate(small, 60, 99, math.inf) + len(x))
    got = _fps_native([small, x], [60, samples], [99, start])                     # and with the small example first
    np.testing.assert_array_equal(got[0], AR.fps_restate(small, 60, 99, math.inf))
    np.testing.assert_array_equal(got[1], ref + 100)


def test_fps_many_examples_two_pass_example_sort():
    B, side, samples = AR.FPS_MANY
    xs = [AR.lattice(side, seed=100 + b) for b in range(B)]
    starts = [(7 * b) % side ** 3 for b in range(B)]
    got = _fps_native(xs, [samples] * B, starts)
    for b in range(B):
        np.testing.assert_array_equal(got[b], AR.fps_restate(xs[b], samples, starts[b], math.inf) + b * side ** 3, err_msg=f"example {b}")


def _fps_cabi(xs, starts, out_ptr, total, max_n, out_len):
    """igs_fps through the C ABI into a sentinel-filled out of out_len entries between two bands; returns out as numpy."""
    L = _lib()
    xyz = _cuda(np.concatenate(xs))
    N, B = xyz.shape[0], len(xs)
    p, st, op = _i32(_ptr([len(x) for x in xs])), _i32(starts), _i32(out_ptr)
    sbytes = L.igs_fps_scratch_bytes(B, N, max_n)
    assert sbytes > 0
    scratch = torch.empty(sbytes, dtype=torch.uint8, device=DEV)
    big, out = _banded(out_len, torch.int64, I64_SENTINEL)
    _ok(L.igs_fps(_stream(), B, N, max_n, xyz.data_ptr(), p.data_ptr(), st.data_ptr(), op.data_ptr(), total, math.inf,
                  scratch.data_ptr(), out.data_ptr()))
    torch.cuda.synchronize()
    assert _bands_intact(big, out_len, I64_SENTINEL)
    return out.cpu().numpy()


def test_fps_contract_total_truncates_the_last_example():
    xs = [AR.lattice(6, seed=1), AR.lattice(7, seed=2)]
    out = _fps_cabi(xs, [3, 4], [0, 20, 50], total=35, max_n=343, out_len=50)
    np.testing.assert_array_equal(out[:20], AR.fps_restate(xs[0], 20, 3, math.inf))
    np.testing.assert_array_equal(out[20:35], AR.fps_restate(xs[1], 15, 4, math.inf) + 216)
    assert (out[35:] == I64_SENTINEL).all(), "an entry past `total` was written"


def test_fps_contract_start_out_of_range_acts_as_zero():
    xs = [AR.lattice(6, seed=3), AR.lattice(5, seed=4)]
    out = _fps_cabi(xs, [-1, 125], [0, 30, 60], total=60, max_n=216, out_len=60)
    np.testing.assert_array_equal(out[:30], AR.fps_restate(xs[0], 30, 0, math.inf))
    np.testing.assert_array_equal(out[30:], AR.fps_restate(xs[1], 30, 0, math.inf) + 216)


def test_fps_contract_empty_example_gets_minus_one():
    xs = [AR.lattice(5, seed=5), AR.lattice(5, seed=5)[:0], AR.lattice(4, seed=6)]
    out = _fps_cabi(xs, [1, 0, 2], [0, 10, 15, 25], total=25, max_n=125, out_len=25)
    np.testing.assert_array_equal(out[:10], AR.fps_restate(xs[0], 10, 1, math.inf))
    np.testing.assert_array_equal(out[10:15], [-1] * 5)
    np.testing.assert_array_equal(out[15:], AR.fps_restate(xs[2], 10, 2, math.inf) + 125)


def test_fps_contract_example_beyond_max_n_gets_minus_one():
    """70 000 points under max_n = 1000 (a launch shaped for 16 leaves of 64): -1 for it, the other example still exact."""
    big = AR.lattice(42, seed=7)[:70000]
    small = AR.lattice(9, seed=8)
    out = _fps_cabi([big, small], [0, 700], [0, 12, 52], total=52, max_n=1000, out_len=52)
    np.testing.assert_array_equal(out[:12], [-1] * 12)
    np.testing.assert_array_equal(out[12:], AR.fps_restate(small, 40, 700, math.inf) + 70000)


# ---------------------------------------------------------------- igs_knn_query
def _knn_native(x, y, k, ptr_x=None, ptr_y=None, weight_scale=None):
    from igs_amd import anchors as A
    px = _i32([0, x.shape[0]] if ptr_x is None else ptr_x)
    py = _i32([0, y.shape[0]] if ptr_y is None else ptr_y)
    idx, d2, w = A.knn_native(_cuda(x), _cuda(y), k, px, py, with_d2=True, weight_scale=weight_scale)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy(), (None if w is None else w.cpu().numpy())


def _check_weights(idx, d2, w, scale):
    """The float64 softmax over the filled slots of the native d2 (test_knn_weights_softmax's rule); empty slots exactly 0."""
    ref = AR.knn_weights_f64(d2, idx, scale)
    print(f"knn weights, k = {idx.shape[1]}, scale {scale}: worst error / bound {float((np.abs(w - ref) / (1e-7 + 1e-5 * np.abs(ref))).max()):.3f}")
    np.testing.assert_allclose(w, ref, rtol=1e-5, atol=1e-7)
    assert (w[idx < 0] == 0).all()
    filled = (idx >= 0).any(1)
    np.testing.assert_allclose(w[filled].sum(1), 1.0, rtol=1e-5)
    assert (w[~filled] == 0).all()


@pytest.mark.parametrize("k", [17, 32, 33])
def test_knn_lattice_bit_equal_32_and_100_slots(k):
    """knnq_kernel<32, false> at both ends of its range and <100, false> below k = 100, on test_knn_lattice_bit_equal's lattices."""
    x = AR.lattice(6, seed=k)
    y = np.concatenate([AR.lattice(5, seed=k + 1, offset=0.5), AR.lattice(3, seed=k + 2, scale=2.0)])
    idx, d2, _ = _knn_native(x, y, k)
    ridx, rd2 = AR.knn_restate(x, y, k)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(d2, rd2)


@pytest.mark.parametrize("k", [16, 32, 100])
def test_knn_masked_instantiations_bit_equal(k):
    """Workgroups 0 and 1 straddle examples (knnq_kernel<K, true>), workgroup 2 does not; example 0 spans two LDS tiles, example 1 has
    40 points: at k = 100 its rows end in -1 / +inf padding with weight 0."""
    x, y, px, py = AR.knn_masked_case(seed=k)
    idx, d2, w = _knn_native(x, y, k, px, py, weight_scale=10.0)
    ridx, rd2 = AR.knn_restate(x, y, k, px, py)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(d2, rd2)
    assert (idx[250:270, 40:] == -1).all() and np.isinf(d2[250:270, 40:]).all()
    _check_weights(idx, d2, w, 10.0)


@pytest.mark.parametrize("ny", [1, 255, 256, 257])
@pytest.mark.parametrize("nx", [2047, 2048, 2049, 4097])
def test_knn_tile_and_workgroup_edges(nx, ny):
    g = np.random.default_rng(nx * 1000 + ny)
    x = g.integers(0, 24, (nx, 3)).astype(np.float32)
    y = g.integers(0, 24, (ny, 3)).astype(np.float32)
    x[-1] = y[0]                                       # the last point of the last tile is query 0's nearest
    idx, d2, _ = _knn_native(x, y, 8)
    ridx, rd2 = AR.knn_restate(x, y, 8)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(d2, rd2)
    assert (idx[0] == nx - 1).any() and d2[0, 0] == 0


@pytest.mark.parametrize("k", [4, 16])
def test_knn_cut_and_non_finite(k):
    """d2 = 99 999^2 is kept, d2 = 1e10 exactly is dropped; NaN / inf rows of x never count; a NaN query has no neighbour."""
    x, y = AR.knn_cut_case()
    idx, d2, w = _knn_native(x, y, k, weight_scale=0.001)
    ridx, rd2 = AR.knn_restate(x, y, k)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(d2, rd2)
    assert (idx[1] == -1).all() and np.isinf(d2[1]).all() and (w[1] == 0).all()
    assert 1 not in idx[0] and not np.isin(idx, [2, 4, 6, 7]).any()
    if k == 16:
        assert 0 in idx[0] and (idx[0] >= 0).sum() == 5
    _check_weights(idx, d2, w, 0.001)
