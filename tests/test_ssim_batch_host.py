"""The batched SSIM of the AGM-Net training loss (igs_amd/csrc/ssim_batch.hip, igs_amd/losses.py) without a GPU: the float64 restatement
against the reference-produced golden file, the refusals of the C ABI before any HIP call, the scratch size, exports and argument counts,
and the routing of the Python layer."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_ssim_batch_scratch_bytes", "igs_ssim_batch_fwd_bwd")
INVALID = -1
FN = "igs_ssim_batch_fwd_bwd"


def test_restatement_reproduces_the_reference_on_a_batch():
    """oracle.torch_losses.ssim_reference_call in float64 against the reference's own float32 `ssim` on a [3, 3, 20, 27] batch (values:
    float32 means of O(1) numbers; gradients: float32 autograd of elements of O(1 / n))."""
    from oracle.torch_losses import ssim_reference_call
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_ssim_batch.npz"))
    assert z["x"].shape == z["gt"].shape == (3, 3, 20, 27) and z["per_image"].shape == (3,)
    gt = torch.from_numpy(z["gt"]).double()
    a = torch.from_numpy(z["x"]).double().requires_grad_(True)
    mean, m = ssim_reference_call(a, gt)
    assert mean.dim() == 0 and m.shape == (3, 3, 20, 27)
    (g,) = torch.autograd.grad(mean, a)
    assert abs(mean.item() - float(z["mean"])) <= 1e-6
    assert np.abs(g.numpy() - z["mean_grad"]).max() <= 1e-5 * np.abs(z["mean_grad"]).max()
    b = torch.from_numpy(z["x"]).double().requires_grad_(True)
    per = ssim_reference_call(b, gt, size_average=False)
    assert per.shape == (3,) and np.abs(per.detach().numpy() - z["per_image"]).max() <= 1e-6
    (g,) = torch.autograd.grad((torch.from_numpy(z["per_image_w"]).double() * per).sum(), b)
    assert np.abs(g.numpy() - z["per_image_grad"]).max() <= 1e-5 * np.abs(z["per_image_grad"]).max()
    assert abs(per.mean().item() - mean.item()) <= 1e-12          # the images weigh the same: the mean of the means is the mean


def _call(L, W=40, H=33, N=2, C=3, pred=64, gt=64, scratch=64, means=64, l1=0, grad=0, smap=0):
    """The entry point on the NULL stream with made-up addresses: every call here must be refused before it reaches HIP."""
    return L.igs_ssim_batch_fwd_bwd(None, W, H, N, C, pred, gt, 1.0, 0.0, scratch, means, l1, grad, smap)


def test_c_abi_refuses_before_any_hip_call():
    from igs_amd import _cabi
    L = _cabi.lib()
    big = dict(W=2048, H=16384, N=1 << 14, C=4)                    # 8 * 2^16 planes * 64 row groups * 64 columns = 2^31
    cases = [(dict(W=0), "positive"), (dict(W=-3), "positive"), (dict(H=0), "positive"), (dict(N=0), "positive"), (dict(C=0), "positive"),
             (dict(N=-1, C=-1), "positive"),
             (dict(pred=0), "NULL"), (dict(gt=0), "NULL"), (dict(scratch=0), "NULL"), (dict(means=0), "NULL"),
             (dict(N=1 << 14, C=5), "IGS_SSIM_BATCH_MAX_PLANES"), (dict(N=65537, C=1), "IGS_SSIM_BATCH_MAX_PLANES"),
             (dict(N=1 << 16, C=1 << 16), "IGS_SSIM_BATCH_MAX_PLANES"),
             (big, "31 bits"), (dict(W=(1 << 31) - 1, H=(1 << 31) - 1, N=1, C=1), "31 bits")]
    for kw, word in cases:
        assert _call(L, **kw) == INVALID, kw
        assert word in _cabi.last_error() and FN in _cabi.last_error(), (kw, _cabi.last_error())
    # the sizes are judged first: a refused size with NULL pointers names the size
    assert _call(L, W=0, pred=0) == INVALID and "positive" in _cabi.last_error()


def test_scratch_bytes():
    from igs_amd import _cabi
    sb = _cabi.lib().igs_ssim_batch_scratch_bytes
    up = lambda n: (n + 255) // 256 * 256
    for W, H, N, C in ((1, 1, 1, 1), (40, 33, 2, 3), (33, 257, 7, 1), (1352, 1014, 32, 3), (97, 65, 1, 5)):
        tiles = ((W + 31) // 32) * ((H + 31) // 32)
        sums = 2 * up(N * C * tiles * 4)                           # a partial SSIM sum and a partial L1 sum per plane and tile
        assert sb(W, H, N, C, 0) == sums, (W, H, N, C)             # no derivative maps without a gradient
        assert sb(W, H, N, C, 1) == sums + up(N * C * 3 * H * W * 4), (W, H, N, C)
    assert sb(1352, 1014, 32, 3, 1) - sb(1352, 1014, 8, 3, 1) == 24 * 3 * (3 * 1352 * 1014 * 4 + 2 * 43 * 32 * 4)
    for bad in ((0, 5, 1, 1), (5, 0, 1, 1), (5, 5, 0, 1), (5, 5, 1, 0), (-1, 5, 1, 1), (5, 5, 65537, 1), (5, 5, 1 << 14, 5),
                (2048, 16384, 1 << 14, 4)):
        assert sb(*bad, 0) == -1 and sb(*bad, 1) == -1, bad
    assert sb(5, 5, 1 << 16, 1, 1) > 0 and sb(2048, 16384 - 32 * 8, 1 << 14, 4, 0) > 0        # the corners of the ranges are in


def test_header_signatures_and_exports_agree():
    from igs_amd import _cabi
    L = _cabi.lib()
    hdr = open(os.path.join(ROOT, "include", "igs_rast.h")).read()
    assert re.search(r"#define IGS_SSIM_BATCH_MAX_PLANES \(1 << 16\)", hdr)
    doc = hdr[hdr.index("SSIM and L1 of a BATCH"):hdr.index("long long igs_ssim_batch_scratch_bytes")]
    assert "loss_utils.py:17-18,33-63" in doc and "main.py:252-265" in doc
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NAMES:
        assert n in _cabi.EXPORTS and hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, plain)
        assert m, n
        assert len(_cabi.SIGNATURES[n][1]) == len(m.group(1).split(",")), n
    assert len(_cabi.SIGNATURES[NAMES[0]][1]) == 5 and len(_cabi.SIGNATURES[NAMES[1]][1]) == 14


def test_python_layer_routing_without_a_gpu():
    """What igs_amd.losses.ssim and l1_ssim refuse can be seen on CPU tensors: every refusal is a NotImplementedError (no fallback)."""
    from igs_amd.losses import l1_ssim, ssim
    x3, x4 = torch.rand(3, 20, 27), torch.rand(2, 3, 20, 27)
    calls = [lambda: ssim(x3, x3, size_average=True),                                   # 3-D inputs with size_average
             lambda: ssim(x4, x4), lambda: ssim(x4, x4, size_average=False),           # CPU tensors
             lambda: ssim(x3, x3.unsqueeze(0), size_average=False),
             lambda: ssim(x4.double(), x4.double()), lambda: ssim(x4.half(), x4.half()), lambda: ssim(x4.bfloat16(), x4.bfloat16()),
             lambda: ssim(x4, x4.clone().requires_grad_(True)),
             lambda: ssim(x4, x4, window_size=7), lambda: ssim(x4, x4[:, :, :, :26]), lambda: ssim(x4, x4[:1]),
             lambda: ssim(x4[:0], x4[:0]),
             lambda: l1_ssim(x4, x4), lambda: l1_ssim(x4[0, 0], x4[0, 0]), lambda: l1_ssim(x4, x4[:1])]
    for f in calls:
        with pytest.raises(NotImplementedError):
            f()


def test_compiled_module_has_the_loss_submodule_and_an_unchanged_top_level():
    from igs_amd import _cabi
    import test_ext_binding_host as T
    E = _cabi.ext()
    assert sorted(n for n in dir(E) if not n.startswith("_")) == sorted(T.PUBLIC)
    assert sorted(n for n in dir(E._loss) if not n.startswith("_")) == ["ssim_batch"]
    line = E._loss.ssim_batch.__doc__.splitlines()[0]
    names = [a.split(": ")[0] for a in line.split("(", 1)[1].rsplit(") -> ", 1)[0].split(", ")]
    assert names == ["a", "b", "c_ssim", "c_l1", "want_grad", "want_map", "want_l1"]
    # the glue refuses on the host what it can: dtype (NotImplementedError), shapes, and tensors that are not on a GPU
    x = torch.rand(2, 3, 8, 9)
    with pytest.raises(NotImplementedError):
        E._loss.ssim_batch(x.double(), x.double(), 1.0, 0.0, True, True, False)
    with pytest.raises(E.RasterizerError, match="shape"):
        E._loss.ssim_batch(x, x[:, :, :, :8], 1.0, 0.0, True, True, False)
    with pytest.raises(E.RasterizerError, match="shape"):
        E._loss.ssim_batch(x[0], x[0], 1.0, 0.0, True, True, False)
    with pytest.raises(E.RasterizerError, match="out of range"):
        E._loss.ssim_batch(x[:0], x[:0], 1.0, 0.0, True, True, False)
    with pytest.raises(E.RasterizerError, match="must be on a GPU"):
        E._loss.ssim_batch(x, x, 1.0, 0.0, True, True, False)
