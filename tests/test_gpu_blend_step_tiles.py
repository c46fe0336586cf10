"""The fused tile kernel (blend_step.hip) against the two-kernel path it must equal bit for bit, on the hand-placed 40 x 24 scenes of
tests/blend_step_case.py: tiles of 0, 1, 64, 65, 128, 129, 192, 193 and 260 instances (the forward at one and two rounds, the
colour-only backward at one, two and three, 64-splat words full, one over and empty), partial tiles on the right and at the bottom,
and a scene in which every pixel saturates long before its list ends.

Three steps of `igs_refine_step` (L1) per scene, with and without `dL_dmean2D` (the |gradient| instance), P divisible by four.  The
library reads IGS_NO_TILE_FUSION once per process, so the two-kernel runs come from ONE child process that runs every case.  Compared
as bits: all 15 image planes and the radii of every step, dL/dmean2D of every step, and parameters and both Adam moments at the end.
The loss value is a float sum over up to 64 shards that the two paths may add in another order: relative 64 * 2^-24.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import blend_step_case as B
from test_gpu_parity import dev  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = [(name, absgrad) for name in sorted(B.LAYOUTS) for absgrad in (False, True)]
LOSS_RTOL = 64 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _two_kernel_runs(tmp):
    assert "IGS_NO_TILE_FUSION" not in os.environ, "this test compares the fused kernel (this process) with the two-kernel path (a child)"
    out = os.path.join(tmp, "two_kernel.npz")
    env = dict(os.environ, IGS_NO_TILE_FUSION="1")
    r = subprocess.run([sys.executable, os.path.abspath(B.__file__), out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _fused_run(name, absgrad):
    return B.run(name, absgrad)


@pytest.fixture(scope="module")
def two_kernel(tmp_path_factory, dev):  # noqa: F811
    return _two_kernel_runs(str(tmp_path_factory.mktemp("blend_step")))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("name,absgrad", CASES, ids=["%s-%s" % (n, "abs" if a else "plain") for n, a in CASES])
def test_fused_step_equals_two_kernel_path_bit_for_bit(dev, two_kernel, name, absgrad):  # noqa: F811
    fused = _fused_run(name, absgrad)
    ref = {k.split("/", 2)[2]: v for k, v in two_kernel.items() if k.startswith("%s/%d/" % (name, int(absgrad)))}
    assert set(ref) == set(fused) and len(fused) >= 4 * B.STEPS + 4
    tiles = B.scene(name)[3]
    assert int(fused["rendered_0"][0]) == sum(tiles), "the layout's instance counts (tests/test_blend_step_isa.py checks them per tile)"
    assert int(fused["abs_instance"][0]) == int(absgrad) and int(ref["abs_instance"][0]) == int(absgrad)
    for k in sorted(fused):
        a, b = fused[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k.startswith("loss_"):
            print("%s %s %s fused %.9g two-kernel %.9g" % (name, absgrad, k, float(a[0]), float(b[0])))
            assert np.isfinite(a).all() and abs(float(a[0]) - float(b[0])) <= LOSS_RTOL * abs(float(b[0])), (k, a, b)
            continue
        differ = int((_bits(a) != _bits(b)).sum())
        assert differ == 0, (name, absgrad, k, "bytes that differ: %d of %d" % (differ, _bits(a).size))
    # the steps did something: a picture, a loss, parameters that moved and moments that are set
    raw = B.scene(name)[0]
    assert np.isfinite(fused["images_0"][0:3]).all() and float(np.abs(fused["images_%d" % (B.STEPS - 1)][0:3]).max()) > 0.05
    assert float(fused["loss_0"][0]) > 0.0
    xyz0 = raw["xyz"].numpy().reshape(-1)
    assert float(np.abs(fused["param"][:xyz0.size] - xyz0).max()) > 0.0 and float(np.abs(fused["exp_avg_sq"]).max()) > 0.0
    if absgrad:
        assert float(np.abs(fused["mean2d_0"]).max()) > 0.0
