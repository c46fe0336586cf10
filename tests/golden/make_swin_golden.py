"""Generates tests/golden/ref_swin.npz: outputs of the reference's own single_head_split_window_attention
(igs/models/unimatch/attention.py) with the mask of its own generate_shift_window_attn_mask (igs/models/unimatch/utils.py), data only.

Run in the build container only (needs the reference checkout):  python tests/golden/make_swin_golden.py REFERENCE_ROOT   (or IGS_REFERENCE in the environment)
The unimatch directory is imported as a package of its own (its __init__ chain above it pulls in the whole model), so the two modules
are read at run time and none of their text is stored.  Cases (h, w, K) = (4, 10, 2) and (6, 9, 3): B = 1, C = 16, float64; q, k, v,
dout, the function's output unshifted and shifted, and autograd's d q / d k / d v of the shifted call for the upstream gradient dout.
C = 16 is enough: the file pins the roll, window and mask logic of tests/window_attention_restatement.py, which is generic in C.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IGS_REFERENCE", "")
CASES = ((4, 10, 2), (6, 9, 3))


def load_unimatch():
    d = os.path.join(REF, "igs", "models", "unimatch")
    spec = importlib.util.spec_from_file_location("ref_unimatch", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["ref_unimatch"] = pkg                                   # (the package's own __init__ is not executed)
    return importlib.import_module("ref_unimatch.attention"), importlib.import_module("ref_unimatch.utils")


def main():
    assert os.path.isdir(REF), "pass the root of the reference checkout"
    att, utils = load_unimatch()
    out = {}
    for h, w, K in CASES:
        g = torch.Generator().manual_seed(1000 * h + 10 * w + K)
        q, k, v, dout = (torch.randn(1, h * w, 16, generator=g, dtype=torch.float64) * s for s in (2.0, 2.0, 1.0, 1.0))
        wh, ww = h // K, w // K
        mask = utils.generate_shift_window_attn_mask((h, w), wh, ww, wh // 2, ww // 2, device=torch.device("cpu")).double()
        tag = "h%d_w%d_K%d_" % (h, w, K)
        plain = att.single_head_split_window_attention(q, k, v, num_splits=K, with_shift=False, h=h, w=w)
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        shifted = att.single_head_split_window_attention(*leaves, num_splits=K, with_shift=True, h=h, w=w, attn_mask=mask)
        grads = torch.autograd.grad(shifted, leaves, dout)
        for name, t in (("q", q), ("k", k), ("v", v), ("dout", dout), ("out", plain), ("out_shift", shifted), ("mask", mask),
                        ("dq", grads[0]), ("dk", grads[1]), ("dv", grads[2])):
            out[tag + name] = t.detach().numpy().astype(np.float64)
    path = os.path.join(HERE, "ref_swin.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
