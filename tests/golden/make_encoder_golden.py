"""Generates tests/golden/ref_encoder.npz: tensors recorded around the norms of the reference's own ResidualBlock and CNNEncoder stem
(igs/models/unimatch/backbone.py) and inputs / outputs of its own feature_add_position (igs/models/unimatch/utils.py), data only.

Run in the build container only (needs the reference checkout):  python tests/golden/make_encoder_golden.py REFERENCE_ROOT   (or IGS_REFERENCE in the environment)
The unimatch directory is imported as a package of its own (its __init__ chain above it pulls in the whole model), so the modules are
read at run time and none of their text is stored.  Everything is float64 with seeded weights:
  ident_*   ResidualBlock(6, 6) at [2, 6, 10, 14]: x (the identity skip), n1_in / n2_in (the tensors entering norm1 / norm2), n1_out
            (relu(norm1(.)), read back from conv2's input), out
  down_*    ResidualBlock(6, 10, stride=2) at [2, 6, 10, 14]: the same plus n3_in (the downsample convolution's output)
  stem_*    conv1 / norm1 / relu1 of CNNEncoder at [2, 3, 20, 12]: n1_in, out (the first 8 of the 64 channels: every plane is normalised
            on its own, and the file stays small)
  pos_C_h_w_K_*   feature_add_position: f0, f1, o0, o1 for (C, h, w, K) = (16, 6, 10, 2), (16, 6, 9, 3), (8, 5, 7, 1)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IGS_REFERENCE", "")
POSITION_CASES = ((16, 6, 10, 2), (16, 6, 9, 3), (8, 5, 7, 1))


def load_unimatch():
    d = os.path.join(REF, "igs", "models", "unimatch")
    spec = importlib.util.spec_from_file_location("ref_unimatch", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["ref_unimatch"] = pkg                                   # (the package's own __init__ is not executed)
    return importlib.import_module("ref_unimatch.backbone"), importlib.import_module("ref_unimatch.utils")


def record_block(block, x, tag, out):
    """Forward hooks: the input of every norm, and conv2's input (= relu(norm1(.)), after the in-place ReLU has run)."""
    seen = {}
    hooks = [block.norm1.register_forward_hook(lambda m, i, o: seen.__setitem__("n1_in", i[0].detach().clone())),
             block.norm2.register_forward_hook(lambda m, i, o: seen.__setitem__("n2_in", i[0].detach().clone())),
             block.conv2.register_forward_hook(lambda m, i, o: seen.__setitem__("n1_out", i[0].detach().clone()))]
    if block.downsample is not None:
        hooks.append(block.downsample[1].register_forward_hook(lambda m, i, o: seen.__setitem__("n3_in", i[0].detach().clone())))
    seen["x"] = x.clone()
    seen["out"] = block(x.clone()).detach().clone()
    for h in hooks:
        h.remove()
    for k, v in seen.items():
        out[tag + k] = v.numpy().astype(np.float64)


def main():
    assert os.path.isdir(REF), "pass the root of the reference checkout"
    backbone, utils = load_unimatch()
    out = {}
    with torch.no_grad():
        torch.manual_seed(11)
        record_block(backbone.ResidualBlock(6, 6).double().eval(), torch.randn(2, 6, 10, 14, dtype=torch.float64) * 2 + 0.5, "ident_", out)
        torch.manual_seed(12)
        record_block(backbone.ResidualBlock(6, 10, stride=2).double().eval(), torch.randn(2, 6, 10, 14, dtype=torch.float64) * 2 + 0.5, "down_", out)
        torch.manual_seed(13)
        enc = backbone.CNNEncoder().double().eval()
        img = torch.randn(2, 3, 20, 12, dtype=torch.float64)
        pre = enc.conv1(img)
        out["stem_n1_in"] = pre[:, :8].clone().numpy().astype(np.float64)
        out["stem_out"] = enc.relu1(enc.norm1(pre))[:, :8].numpy().astype(np.float64)
        for C, h, w, K in POSITION_CASES:
            g = torch.Generator().manual_seed(1000 * C + 100 * h + 10 * w + K)
            f0, f1 = (torch.randn(2, C, h, w, generator=g, dtype=torch.float64) for _ in range(2))
            o0, o1 = utils.feature_add_position(f0, f1, K, C)
            tag = "pos_%d_%d_%d_%d_" % (C, h, w, K)
            for name, t in (("f0", f0), ("f1", f1), ("o0", o0), ("o1", o1)):
                out[tag + name] = t.numpy().astype(np.float64)
    path = os.path.join(HERE, "ref_encoder.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
