"""The eigen-solver of the plane fit, branch by branch: hyp() (geom_math.h) is written with selects instead of its two arms, "same
operations on the same operands, same bits".  tests/golden/eigen_branches.npz holds a hand-made scene (inputs and camera stored in the
file) and the records the preprocess kernel wrote for it while hyp() still had the reference's two arms
(tests/golden/make_eigen_branches_golden.py); the forward must reproduce every record word.

Every floating-point operation on the way to a record is separately rounded (contraction off) and IEEE (divide, square root): the
expected words do not depend on how the compiler schedules them, so the comparison is for equality.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "eigen_branches.npz")


@pytest.fixture(scope="module")
def scene():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def sigma32(s, q):
    """Sigma = R diag(s^2) R^T with every product and sum rounded to float32 in the order of cov3d_from_scale_rot (geom_math.h)."""
    f = np.float32
    r, x, y, z = (f(v) for v in q)
    one, two = f(1), f(2)
    R = [[one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)],
         [two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)],
         [two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]]
    M = [[f(s[k]) * R[i][k] for k in range(3)] for i in range(3)]
    S = np.zeros((3, 3), np.float32)
    for i in range(3):
        for j in range(3):
            S[i, j] = M[i][0] * M[j][0] + M[i][1] * M[j][1] + M[i][2] * M[j][2]
    return S


def near0(v):
    return abs(np.float32(v)) <= np.float32(0.0000001)


def test_every_hand_placed_case_reaches_its_branch(scene):
    """On the CPU: the named Gaussians take the branch of eig_sym3 / cov2d_planes_eig that their name says (conditions restated from
    geom_math.h on a float32 Sigma; the smallest eigenvalue from the oracle's solver, the plain-C form of the same algorithm)."""
    from oracle import c_oracle as co
    names = [str(n) for n in scene["names"]]
    seen = set()
    with co.thread_precision("float32"):
        for i, n in enumerate(names):
            if n.startswith("generic_"):
                continue
            seen.add(n)
            S = sigma32(scene["scales"][i], scene["rotations"][i])
            skip_row2 = near0(abs(S[2, 0]) + abs(S[2, 1]))            # Householder: near0(scale)
            ok, val, _ = co.eig_sym3(S)
            assert ok == 3, (n, ok)
            evmin = float(val.min())
            if n in ("householder_near0_no_sweep", "equal_scales_no_sweep", "rank_deficient_axis"):
                assert skip_row2 and near0(S[1, 0]), (n, S)              # e0 = a10, e1 = a21: QL finds nothing to do
            elif n == "householder_near0_sweeps":
                assert skip_row2 and not near0(S[1, 0]), (n, S)          # ... QL sweeps on e0 only (m = 1)
            else:
                assert not skip_row2, (n, S)                             # full Householder step, both QL loops
            if n.startswith("rank_deficient"):
                assert evmin <= 1e-8, (n, evmin)                         # Sigma^-1 := e_min e_min^T
            else:
                assert evmin > 1e-8, (n, evmin)
    assert seen == {"householder_near0_no_sweep", "equal_scales_no_sweep", "householder_near0_sweeps", "rotated_sweeps",
                    "rank_deficient_axis", "rank_deficient_rotated", "regular_thin_rotated"}
    # the generic ones all take the full Householder step and sweep: neighbouring lanes disagree in hyp() about which magnitude is larger
    for i, n in enumerate(names):
        if n.startswith("generic_"):
            S = sigma32(scene["scales"][i], scene["rotations"][i])
            assert not near0(abs(S[2, 0]) + abs(S[2, 1])), n
    assert len(names) > 256                                              # more than one workgroup


@pytest.mark.gpu
def test_records_keep_their_bits(scene):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_eigen_branches_golden as G
    rec, radii = G.forward_records(scene, torch.device("cuda:0"))
    np.testing.assert_array_equal(radii, scene["radii"])
    assert (radii > 0).all()
    want = scene["rec"]
    bad = np.argwhere(rec != want)
    assert bad.size == 0, ("record words that changed (Gaussian, word): %s ..." % bad[:8].tolist(),
                           [str(scene["names"][i]) for i in sorted(set(bad[:8, 0].tolist()))])
