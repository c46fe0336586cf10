"""simple_knn.distCUDA2 on the GPU (knn.hip: igs_knn_mean_dist2) against the restatement of tests/knn_restatement.py: parity with a
float64 brute force, bit-equality on lattices, N <= 3, large clouds, determinism, permutation equivariance, non-finite points,
strided input on a side stream, and create_from_pcd (igs_amd.io.gaussians_from_point_cloud) through one rendered frame."""
import numpy as np
import pytest
import torch

import knn_restatement as KR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _knn(x):
    from simple_knn._C import distCUDA2
    out = distCUDA2(x)
    torch.cuda.synchronize()
    return out


def _uniform(n, seed=0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 3, generator=g) + offset).float()


def _clustered(n, seed=0, outliers=0.01, blobs=12, far=1000.0):
    """Gaussian blobs of different widths plus a fraction of far outliers (a COLMAP cloud with sky points)."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(blobs, 3, generator=g) * 3.0
    widths = torch.rand(blobs, generator=g) * 0.3 + 0.01
    k = torch.randint(0, blobs, (n,), generator=g)
    x = centres[k] + torch.randn(n, 3, generator=g) * widths[k, None]
    m = int(n * outliers)
    if m:
        d = torch.nn.functional.normalize(torch.randn(m, 3, generator=g), dim=1)
        x[torch.randperm(n, generator=g)[:m]] = d * (far * (1 + torch.rand(m, 1, generator=g)))
    return x.float()


def _check_parity(x, out):
    truth = KR.brute_f64(x.to(DEV)).cpu()
    out = out.cpu().double()
    zero = truth == 0
    assert torch.all(out[zero] == 0), "exact 0 where the truth is 0"
    rel = ((out - truth).abs() / truth.clamp_min(1e-300))[~zero]
    assert rel.numel() == 0 or rel.max().item() <= 2e-6, rel.max().item()


@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 1000, 4097, 20000])
def test_uniform_cube_parity(n):
    x = _uniform(n, seed=n)
    _check_parity(x, _knn(x.to(DEV)))


def test_clustered_with_outliers_parity():
    x = _clustered(50000)
    _check_parity(x, _knn(x.to(DEV)))


def test_line_plane_offset_duplicates_parity():
    g = torch.Generator().manual_seed(3)
    t = torch.rand(5000, 1, generator=g)
    line = (torch.tensor([[0.3, -1.2, 2.0]]) + t * torch.tensor([[1.0, 2.0, -0.5]])).float()
    uv = torch.rand(6000, 2, generator=g)
    plane = (uv[:, :1] * torch.tensor([[1.0, 0.0, 1.0]]) + uv[:, 1:] * torch.tensor([[0.0, 1.0, -1.0]])).float()
    offset = _uniform(8000, seed=4, offset=1e3)
    base = _uniform(700, seed=5)
    dup = torch.cat([base, base, base[:300], base[:50]])[torch.randperm(1750, generator=g)]
    for x in (line, plane, offset, dup):
        _check_parity(x, _knn(x.to(DEV)))


def test_integer_lattice_bit_equal_to_restatement():
    x = KR.lattice(16)
    perm = np.random.default_rng(0).permutation(len(x))
    x = x[perm]
    out = _knn(torch.from_numpy(x).to(DEV)).cpu().numpy()
    np.testing.assert_array_equal(out, KR.restate_f32(x))
    assert np.all(out == 1.0)


def test_small_n_exact_values():
    fmax3 = np.float32(KR.FLT_MAX) / np.float32(3)
    assert _knn(torch.empty(0, 3, device=DEV)).shape == (0,)
    assert torch.isinf(_knn(torch.zeros(1, 3, device=DEV))).all()
    assert torch.isinf(_knn(torch.tensor([[0.0, 0, 0], [1, 2, 3]], device=DEV))).all()
    out = _knn(torch.tensor([[0.0, 0, 0], [1, 2, 3], [-1, 0.5, 2]], device=DEV)).cpu().numpy()
    np.testing.assert_array_equal(out, np.full(3, fmax3, np.float32))
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]], np.float32)
    np.testing.assert_array_equal(_knn(torch.from_numpy(x).to(DEV)).cpu().numpy(), KR.restate_f32(x))


@pytest.mark.parametrize("kind,n", [("uniform", 2_000_000), ("clustered", 1_000_000)])
def test_large_clouds_at_random_queries(kind, n):
    x = (_uniform(n, seed=11) if kind == "uniform" else _clustered(n, seed=12)).to(DEV)
    out = _knn(x)
    q = torch.randperm(n, generator=torch.Generator().manual_seed(13))[:4096].to(DEV)
    truth = KR.brute_f64(x, q, chunk=16)
    got = out[q].double()
    zero = truth == 0
    assert torch.all(got[zero] == 0)
    rel = ((got - truth).abs() / truth.clamp_min(1e-300))[~zero]
    assert rel.max().item() <= 2e-6, rel.max().item()
    assert torch.isfinite(out).all()


def test_repeat_bit_identical_and_permutation_equivariant():
    x = _clustered(100000, seed=21).to(DEV)
    a, b = _knn(x), _knn(x)
    assert torch.equal(a, b)
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(22)).to(DEV)
    assert torch.equal(_knn(x[perm]), a[perm])
    y = _uniform(30000, seed=23).to(DEV)
    perm = torch.randperm(y.shape[0], generator=torch.Generator().manual_seed(24)).to(DEV)
    assert torch.equal(_knn(y[perm]), _knn(y)[perm])


def test_non_finite_points_never_become_neighbours():
    x = _uniform(5000, seed=31)
    bad = torch.tensor([17, 400, 401, 2500, 4999])
    vals = [float("nan"), float("inf"), -float("inf"), float("nan"), float("inf")]
    y = x.clone()
    for i, v in zip(bad.tolist(), vals):
        y[i, i % 3] = v
    y[1234] = float("nan")
    bad = torch.cat([bad, torch.tensor([1234])])
    keep = torch.ones(5000, dtype=torch.bool)
    keep[bad] = False
    got = _knn(y.to(DEV)).cpu()
    ref = _knn(x[keep].to(DEV)).cpu()
    assert torch.equal(got[keep], ref)
    # a cloud with only a few finite points among non-finite ones: no fault, finite points keep their exact values
    z = torch.full((300, 3), float("nan"))
    z[::50] = _uniform(6, seed=32)
    got = _knn(z.to(DEV)).cpu()
    assert torch.equal(got[::50], _knn(z[::50].to(DEV)).cpu())


def test_strided_input_on_a_side_stream():
    from simple_knn._C import distCUDA2
    base = _uniform(40000, seed=41)
    wide = torch.zeros(40000, 6)
    wide[:, ::2] = base
    ref = _knn(base.to(DEV))
    s = torch.cuda.Stream(device=DEV)
    src = wide.to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(20_000_000)                # keeps s busy: work on any other stream would run ahead and see no input
        x = src * 1.0                                    # written on s after the sleep
        out = distCUDA2(x[:, ::2])
        done = s.record_event()
    s.synchronize()
    assert done.query()
    assert torch.equal(out, ref)


def test_gaussians_from_point_cloud_and_one_frame():
    from igs_amd.io import gaussians_from_point_cloud
    from igs_amd.refine import GaussianParams
    from igs_amd.scenes import cfg1_scene
    from diff_gaussian_rasterization_rade import GaussianRasterizationSettings, GaussianRasterizer
    g = torch.Generator().manual_seed(51)
    xyz = (torch.rand(3000, 3, generator=g) * 3.0 - 1.5).float()
    rgb = torch.randint(0, 256, (3000, 3), generator=g).float() / 255.0
    raw = gaussians_from_point_cloud(xyz, rgb, DEV)
    want = KR.create_from_pcd(xyz.to(DEV), rgb.to(DEV), _knn(xyz.to(DEV)))
    for k in ("xyz", "rotation", "shs", "opacity", "scaling"):
        assert raw[k].shape == want[k].shape and raw[k].device.type == "cuda", k
        assert torch.equal(raw[k], want[k]), k
    assert raw["shs"].shape == (3000, 16, 3) and torch.all(raw["shs"][:, 1:] == 0)
    assert torch.allclose(raw["opacity"], torch.full_like(raw["opacity"], float(np.log(0.1 / 0.9))))
    truth = KR.brute_f64(xyz.to(DEV)).clamp_min(1e-7)
    assert torch.allclose(raw["scaling"][:, 0].double(), 0.5 * torch.log(truth), rtol=0, atol=1e-5)

    params = GaussianParams(raw, DEV)
    a = params.activated()
    _, cams, bg = cfg1_scene(P=10, size=128)
    cam = cams[0].to(DEV)
    settings = GaussianRasterizationSettings(
        image_height=cam.height, image_width=cam.width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, kernel_size=0.0,
        bg=bg.to(DEV), scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
        sh_degree=3, campos=cam.camera_center, prefiltered=False, require_depth=True, require_coord=True, debug=False)
    with torch.no_grad():
        color, radii = GaussianRasterizer(settings)(means3D=a["means3D"], means2D=torch.zeros_like(a["means3D"]),
                                                    opacities=a["opacities"], shs=a["shs"], scales=a["scales"],
                                                    rotations=a["rotations"])[:2]
    torch.cuda.synchronize()
    assert color.shape == (3, 128, 128) and torch.isfinite(color).all()
    assert (radii > 0).sum().item() > 1000 and color.abs().sum().item() > 0
