"""The multi-view anchor feature lift without a GPU: both float64 restatements (tests/lift_restatement.py) against the outputs of the
reference's own perspective_projection (tests/golden/ref_lift.npz, made by tests/golden/make_lift_golden.py), and the argument refusals
of the C ABI, the compiled module and the Python layer (igs_amd/csrc/lift.hip, igs_amd/motion.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import lift_restatement as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("igs_anchor_lift_scratch_bytes", "igs_anchor_lift_bwd_scratch_bytes", "igs_anchor_lift_fwd", "igs_anchor_lift_bwd")


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_lift.npz"))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _intr4(K):
    return torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1)


# ---------------------------------------------------------------- the restatements against the reference's outputs
def test_restatements_match_the_reference_forward(fx):
    """The reference computed in float32, so the float64 restatements must lie within the derived float32 bound of its output."""
    feat, pts, w2c, intr = fx["feat"], fx["points"], fx["w2c"], _intr4(fx["intrinsics"])
    bound = LR.forward_bound(feat, pts, w2c, intr)
    a = LR.lift_restate(feat.double(), pts.double(), w2c.double(), intr.double())
    b = LR.lift_grid_sample(feat.double(), pts.double(), w2c.double(), intr.double())
    ref = fx["out"].double()
    assert a.shape == ref.shape == (2, 96, 5)
    print("max |restatement - reference| =", (a - ref).abs().max().item(), "| max bound =", bound.max().item(), "| max |ref| =", ref.abs().max().item())
    assert ((a - ref).abs() <= bound).all()
    assert ((b - ref).abs() <= bound).all()
    assert ((a - b).abs() <= 1e-12 * (1 + ref.abs())).all()              # the two float64 statements agree with each other
    assert (ref != 0).float().mean() > 0.3                                 # (a real case: many samples inside)
    # not vacuous: the same bound rejects align_corners=True
    wrong = LR.lift_restate(feat.double(), pts.double(), w2c.double(), intr.double(), align_corners=True)
    assert not ((wrong - ref).abs() <= bound).all()


def test_restatement_backward_matches_the_reference_autograd(fx):
    feat, pts, w2c, intr = fx["feat"], fx["points"], fx["w2c"], _intr4(fx["intrinsics"])
    x = feat.double().requires_grad_(True)
    LR.lift_restate(x, pts.double(), w2c.double(), intr.double()).backward(fx["gout"].double())
    tol = LR.backward_bound(fx["gout"], pts, w2c, intr, 12, 20)
    assert ((x.grad - fx["dfeat"].double()).abs() <= tol).all()
    assert (fx["dfeat"] != 0).any()


def test_fixture_pins_the_swapped_names_and_fov2focal(fx):
    """The fixture's intrinsics were built by GridEncoder's rule with the reference's fov2focal on a 12 x 20 map: fx from shape[-2]."""
    fovx, fovy = fx["fov"].tolist()
    k = LR.grid_encoder_intr((6, 5, 12, 20), fovx, fovy, 6)
    assert torch.equal(k.float(), _intr4(fx["intrinsics"]))
    assert k[0, 2].item() == 6.0 and k[0, 3].item() == 10.0              # cx = H / 2, cy = W / 2: the swap
    assert abs(fx["focal"][0].item() - 12 / (2 * math.tan(fovx / 2))) < 1e-12


def test_restatement_by_hand():
    """One view, identity pose, a 2 x 2 map: a sample at the centre averages the four pixels; one at a pixel centre returns it; a
    sample half a pixel outside takes half of the edge pixels; the view mean divides by V even when a view adds nothing."""
    feat = torch.tensor([[[[1.0, 2.0], [3.0, 4.0]]]], dtype=torch.float64)
    w2c = torch.eye(4, dtype=torch.float64).unsqueeze(0)
    intr = torch.tensor([[1.0, 1.0, 0.0, 0.0]], dtype=torch.float64)     # u = x / z, v = y / z; ix = u - 0.5
    pts = torch.tensor([[[1.0, 1.0, 1.0], [0.5, 0.5, 1.0], [0.0, 0.5, 1.0], [-1.0, -1.0, -1.0], [5.0, 5.0, 1.0], [1.0, 1.0, 0.0]]],
                       dtype=torch.float64)
    out = LR.lift_restate(feat, pts, w2c, intr)
    assert out[0, :, 0].tolist() == [2.5, 1.0, 0.5, 2.5, 0.0, 0.0]       # (z < 0 mirrors onto the centre; z = 0 is not finite: zero)
    two = LR.lift_restate(torch.cat([feat, feat * 0]), pts, w2c.repeat(2, 1, 1), intr.repeat(2, 1))
    assert two[0, :, 0].tolist() == [1.25, 0.5, 0.25, 1.25, 0.0, 0.0]


# ---------------------------------------------------------------- the C ABI
def test_cabi_refuses_bad_arguments_before_any_hip_call():
    """IGS_RAST_E_INVALID (-1) with a message, never IGS_RAST_E_HIP (-2): without a GPU any HIP call would fail."""
    from igs_amd import _cabi
    L = _cabi.lib()
    for name in NAMES:
        assert name in _cabi.EXPORTS and hasattr(L, name)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    err = _cabi.last_error

    def fwd(B=1, V=4, A=10, Cc=8, H=16, W=16, dt=0, fs=None, os_=None, ptrs=None):
        fs = fs or (Cc * H * W, H * W, W, 1)
        os_ = os_ or (1, A)
        ptrs = ptrs or [p] * 6                                           # feat, points, w2c, intr, out, scratch
        return L.igs_anchor_lift_fwd(None, B, V, A, Cc, H, W, dt, ptrs[0], *fs, ptrs[1], ptrs[2], ptrs[3], ptrs[4], *os_, ptrs[5])

    def bwd(B=1, V=4, A=10, Cc=8, H=16, W=16, dt=0, fs=None, gs=None, ptrs=None):
        fs = fs or (Cc * H * W, H * W, W, 1)
        gs = gs or (1, A)
        ptrs = ptrs or [p] * 6                                           # points, w2c, intr, dout, dfeat, scratch
        return L.igs_anchor_lift_bwd(None, B, V, A, Cc, H, W, dt, ptrs[0], ptrs[1], ptrs[2], ptrs[3], *gs, ptrs[4], *fs, ptrs[5])

    bad = ((dict(B=-1), "B out of range"), (dict(V=0), "V out of range"), (dict(V=17), "V out of range"), (dict(A=-1), "A out of range"),
           (dict(Cc=0), "C out of range"), (dict(Cc=1025), "C out of range"), (dict(H=0), "H out of range"), (dict(H=2049), "H out of range"),
           (dict(W=0), "W out of range"), (dict(W=2049), "W out of range"), (dict(B=3, A=(1 << 24) // 3 + 1), "B * A out of range"),
           (dict(B=5, V=16, H=512, W=512), "B * V * H * W out of range"), (dict(dt=2), "dtype"), (dict(dt=-1), "dtype"))
    for kw, what in bad:
        assert fwd(**kw) == -1 and what in err(), (kw, err())
        assert bwd(**kw) == -1 and what in err(), (kw, err())
        k = dict(B=1, V=4, A=10, Cc=8, H=16, W=16, dt=0)
        k.update(kw)
        assert L.igs_anchor_lift_scratch_bytes(k["B"], k["V"], k["A"], k["Cc"], k["H"], k["W"], k["dt"]) == 0
        assert L.igs_anchor_lift_bwd_scratch_bytes(k["B"], k["V"], k["A"], k["Cc"], k["H"], k["W"], k["dt"]) == 0
    # the limits themselves are accepted (sizes only: the scratch functions make no HIP call)
    assert L.igs_anchor_lift_scratch_bytes(1, 16, 1 << 24, 1024, 512, 2048, 1) >= 16 * (1 << 24) * 12
    assert L.igs_anchor_lift_scratch_bytes(1, 1, 1, 1, 2048, 2048, 0) > 0
    # strides: channels-last and other patterns are refused with their own messages; slices of n and c are fine
    assert fwd(fs=(8 * 256, 1, 16 * 8, 8)) == -1 and "channels-last" in err()
    assert bwd(fs=(8 * 256, 1, 16 * 8, 8)) == -1 and "channels-last" in err()
    assert fwd(fs=(8 * 512, 512, 32, 2)) == -1 and "plane must be contiguous" in err()
    assert fwd(fs=(8 * 256, 256, 17, 1)) == -1 and "plane must be contiguous" in err()
    assert fwd(fs=(-1, 256, 16, 1)) == -1 and "negative" in err()
    assert bwd(fs=(8 * 256, 255, 16, 1)) == -1 and "overlap" in err()
    assert fwd(os_=(2, 10)) == -1 and "output strides" in err()
    assert bwd(gs=(8, 2)) == -1 and "d out strides" in err()
    for i in range(6):
        ptrs = [p] * 6
        ptrs[i] = None
        assert fwd(ptrs=ptrs) == -1 and "NULL" in err(), i
        assert bwd(ptrs=ptrs) == -1 and "NULL" in err(), i
    # nothing to do: 0 without a launch
    assert fwd(A=0, ptrs=[None] * 6) == 0 and fwd(B=0, ptrs=[None] * 6) == 0
    assert fwd(A=0, os_=(1, 0)) == 0
    assert bwd(B=0, ptrs=[None] * 6) == 0
    # scratch sizes: the table is 12 bytes per sample; the backward adds 64 bytes per sample of sort buffers and the pixel starts
    S, NPIX = 5 * 4 * 8192, 5 * 4 * 128 * 128
    f = L.igs_anchor_lift_scratch_bytes(5, 4, 8192, 128, 128, 128, 0)
    b = L.igs_anchor_lift_bwd_scratch_bytes(5, 4, 8192, 128, 128, 128, 0)
    assert 12 * S <= f <= 12 * S + 4096
    assert b >= f + 64 * S + 4 * (NPIX + 1)


def test_header_states_the_limits_and_version_is_unchanged():
    h = open(os.path.join(ROOT, "include", "igs_rast.h")).read()
    for s in ("#define IGS_LIFT_MAX_C 1024", "#define IGS_LIFT_MAX_V 16", "#define IGS_LIFT_MAX_HW 2048",
              "#define IGS_LIFT_MAX_PIXELS (1 << 24)", "#define IGS_LIFT_MAX_SAMPLES (1 << 24)"):
        assert s in h
    for name in NAMES:
        assert name + "(" in h
    from igs_amd import _cabi
    assert _cabi.lib().igs_rast_version() == 4


# ---------------------------------------------------------------- the compiled module and the Python layer
def test_compiled_module_refusals():
    from igs_amd import _cabi
    E = _cabi.ext()
    feat, pts, w2c, intr = torch.zeros(4, 8, 16, 16), torch.zeros(1, 10, 3), torch.eye(4).repeat(4, 1, 1), torch.ones(4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.motion_lift_fwd(feat, pts, w2c, intr)
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        E.motion_lift_fwd(feat.double(), pts, w2c, intr)
    with pytest.raises(NotImplementedError, match="anchor_points must be"):
        E.motion_lift_fwd(feat, pts.double(), w2c, intr)
    with pytest.raises(RuntimeError, match="shape"):
        E.motion_lift_fwd(feat, torch.zeros(1, 10, 2), w2c, intr)
    with pytest.raises(RuntimeError, match="shape"):
        E.motion_lift_fwd(feat, pts, w2c, torch.ones(3, 4))
    with pytest.raises(RuntimeError, match="views"):
        E.motion_lift_fwd(feat, torch.zeros(3, 10, 3), w2c, intr)
    with pytest.raises(RuntimeError, match="out of range"):
        E.motion_lift_fwd(torch.zeros(4, 1025, 2, 2), pts, w2c, intr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.motion_lift_bwd(torch.zeros(1, 8, 10), pts, w2c, intr, 16, 16)
    with pytest.raises(RuntimeError, match="shape"):
        E.motion_lift_bwd(torch.zeros(1, 8, 11), pts, w2c, intr, 16, 16)


def test_python_layer_refusals():
    from igs_amd import motion
    feat, pts, c2w = torch.zeros(4, 8, 16, 16), torch.zeros(1, 10, 3), torch.eye(4).repeat(4, 1, 1)
    K = torch.eye(3).repeat(4, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        motion.lift_anchor_features(feat, pts, c2w, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        motion.grid_encoder_lift(feat, pts, torch.ones(1, 2), c2w.reshape(1, 4, 4, 4))
    with pytest.raises(NotImplementedError, match="float32 or float16"):
        motion.lift_anchor_features(feat.bfloat16(), pts, c2w, K)
    with pytest.raises(NotImplementedError, match="float32"):
        motion.lift_anchor_features(feat, pts.double(), c2w, K)
    with pytest.raises(ValueError, match="motion_feature must be"):
        motion.lift_anchor_features(feat[0], pts, c2w, K)
    with pytest.raises(ValueError, match="anchor_points must be"):
        motion.lift_anchor_features(feat, pts[0], c2w, K)
    with pytest.raises(ValueError, match="c2ws must be"):
        motion.lift_anchor_features(feat, pts, c2w[:3], K)
    with pytest.raises(ValueError, match="c2w_input must be"):
        motion.grid_encoder_lift(feat, pts, torch.ones(1, 2), c2w)
