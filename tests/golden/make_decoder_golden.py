"""Generates tests/golden/ref_decoder.npz: outputs of the reference's own MLP (igs/models/networks.py) with output heads built the way
GS3DRenderer.configure builds them (igs/models/gs.py:543-559: one nn.Linear(in_channels, ch) per feature), data only.

Run in the build container only (needs the reference checkout):  python tests/golden/make_decoder_golden.py REFERENCE_ROOT   (or IGS_REFERENCE in the environment)
networks.py does not import here (einops, icecream, the igs package), so only the AST nodes of the class MLP and of the function
get_activation (igs/utils/ops.py) are compiled; the reference is read at run time and none of its text is stored.  The heads get random
weights: the shipped initialisation is zero weights, which would pin nothing.

Cases, float64, N = 40:
  case0: MLP(dim_in 20, dim_out 24, n_neurons 24, n_hidden_layers 2, silu), heads (3, 4)
  case1: MLP(dim_in 16, dim_out 32, n_neurons 32, n_hidden_layers 1, relu), heads (5,)
Stored per case: x, every MLP and head parameter under its state_dict() key, act_after (per Linear of the MLP: is the next layer an
activation), the activation's name, and one output per head, computed as decode_residual_feature does (gs.py:858-869).
"""
import ast
import os
import sys
import typing

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IGS_REFERENCE", "")
N = 40
CASES = [dict(dim_in=20, dim_out=24, n_neurons=24, n_hidden_layers=2, activation="silu", heads=(3, 4)),
         dict(dim_in=16, dim_out=32, n_neurons=32, n_hidden_layers=1, activation="relu", heads=(5,))]


def load_nodes(path, kind, names, env):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, kind) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), [n.name for n in body]
    exec(compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), path, "exec"), env)
    return env


def main():
    assert os.path.isdir(REF), "pass the root of the reference checkout"
    torch.set_default_dtype(torch.float64)
    env = {"torch": torch, "nn": nn, "F": F, "Optional": typing.Optional, "Callable": typing.Callable}
    load_nodes(os.path.join(REF, "igs", "utils", "ops.py"), ast.FunctionDef, ["get_activation"], env)
    load_nodes(os.path.join(REF, "igs", "models", "networks.py"), ast.ClassDef, ["MLP"], env)
    out = {}
    for i, case in enumerate(CASES):
        torch.manual_seed(50 + i)
        kw = {k: v for k, v in case.items() if k != "heads"}
        mlp = env["MLP"](**kw)
        heads = nn.ModuleList([nn.Linear(case["dim_out"], ch) for ch in case["heads"]])          # configure's loop, default init kept
        x = torch.randn(N, case["dim_in"])
        tag = "case%d." % i
        out[tag + "x"] = x.numpy()
        for k, v in mlp.state_dict().items():
            out[tag + "mlp." + k] = v.numpy()
        for k, v in heads.state_dict().items():
            out[tag + "heads." + k] = v.numpy()
        mods = list(mlp.layers)
        out[tag + "act_after"] = np.array([int(j + 1 < len(mods) and not isinstance(mods[j + 1], nn.Linear))
                                           for j, m in enumerate(mods) if isinstance(m, nn.Linear)])
        out[tag + "linear_index"] = np.array([j for j, m in enumerate(mods) if isinstance(m, nn.Linear)])
        out[tag + "activation"] = np.array(case["activation"])
        with torch.no_grad():
            feat = mlp(x)
            for k, layer in enumerate(heads):
                out[tag + "out%d" % k] = layer(feat).numpy()
    path = os.path.join(HERE, "ref_decoder.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
