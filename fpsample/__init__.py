"""Drop-in for `fpsample.bucket_fps_kdline_sampling` (igs/models/gs.py:14 `import fpsample`; get_mask_fpsample, gs.py:983), backed
by the MI355X-native HIP library (igs_amd/csrc/anchors.hip).

The bucket/kd-line FPS of fpsample is an exact farthest-point sampling, so this is vanilla FPS on the GPU: initial distance +inf,
ties to the lowest index.  `h` (the kd-tree height) is validated and otherwise unused, because an exact FPS does not depend on it.
`start_idx=None` draws the start with `np.random.randint(N)`: a deliberate, seedable choice.
Only float32 [N, 3] arrays are supported (NotImplementedError otherwise); the points go to the current GPU and back.
"""
import math

import numpy as np
import torch

from igs_amd import anchors as _A

__all__ = ["bucket_fps_kdline_sampling"]


def bucket_fps_kdline_sampling(pc, n_samples, h, start_idx=None):
    """Indices (numpy int64 [n_samples], selection order) of a farthest-point sampling of the numpy [N, 3] float32 array pc."""
    pc = np.asarray(pc)
    if pc.ndim != 2 or pc.shape[1] != 3:
        raise NotImplementedError(f"fpsample.bucket_fps_kdline_sampling: only [N, 3] point arrays are supported (got {list(pc.shape)})")
    if pc.dtype != np.float32:
        raise NotImplementedError(f"fpsample.bucket_fps_kdline_sampling: only float32 points are supported (got {pc.dtype})")
    if isinstance(h, bool) or not isinstance(h, (int, np.integer)) or h < 1:
        raise ValueError(f"fpsample.bucket_fps_kdline_sampling: h must be a positive integer (got {h!r})")
    N = pc.shape[0]
    n_samples = int(n_samples)
    if n_samples < 0 or n_samples > N:
        raise ValueError(f"fpsample.bucket_fps_kdline_sampling: n_samples = {n_samples} is not in [0, N = {N}]")
    if start_idx is None:
        start = int(np.random.randint(N)) if N > 0 else 0
    else:
        start = int(start_idx)
        if not 0 <= start < N:
            raise ValueError(f"fpsample.bucket_fps_kdline_sampling: start_idx = {start} is not in [0, {N})")
    if n_samples == 0:
        return np.zeros(0, dtype=np.int64)
    if not torch.cuda.is_available():
        raise RuntimeError("fpsample.bucket_fps_kdline_sampling: needs a GPU (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.from_numpy(np.ascontiguousarray(pc)).to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    out = _A.fps_native(x, torch.tensor([0, N], **i32), torch.tensor([start], **i32), torch.tensor([0, n_samples], **i32), n_samples, N,
                        math.inf)
    return out.cpu().numpy()
