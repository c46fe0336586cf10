"""Generates tests/golden/ref_token_ops.npz: outputs and autograd gradients of the reference's own TransformerLayer
(igs/models/unimatch/transformer.py) and BasicTransformerBlock with its FeedForward and GEGLU (igs/models/transformers.py), data only.

Run in the build container only (needs the reference checkout):  python tests/golden/make_token_ops_golden.py REFERENCE_ROOT   (or IGS_REFERENCE in the environment)
Neither file imports here (diffusers, the igs package), so only the AST nodes of the classes TransformerLayer, and
MemoryEfficientAttentionMixin, GEGLU, FeedForward, BasicTransformerBlock are compiled; the reference is read at run time and none of its
text is stored.  The layer gets the reference's own attention functions (igs/models/unimatch/attention.py, imported as make_swin_golden.py
does) and the mask of its own generate_shift_window_attn_mask; the block gets an identity maybe_allow_in_graph and, for
diffusers' Attention, the one-Linear stand-in of tests/token_ops_restatement.py: the file pins the wiring around the attention, not the
attention.

Cases, float64: TransformerLayer(d_model=16) with no_ffn True and False, with_shift both, B = 2, h x w = 4 x 6, K = 2, LayerNorm weights
and biases randomised away from 1 / 0; BasicTransformerBlock(16, 2, 8) on [2, 10, 16].  Stored per case: inputs, every parameter under its
state_dict() key, the output, and autograd's gradients to the inputs and to every parameter for a fixed upstream gradient.
"""
import ast
import importlib
import importlib.util
import os
import sys
import typing

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import token_ops_restatement as TR  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IGS_REFERENCE", "")
B, H, W, K, DIM = 2, 4, 6, 2, 16


def load_classes(path, names, env):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), [n.name for n in body]
    exec(compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), path, "exec"), env)
    return env


def load_unimatch():
    d = os.path.join(REF, "igs", "models", "unimatch")
    spec = importlib.util.spec_from_file_location("ref_unimatch", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    sys.modules["ref_unimatch"] = importlib.util.module_from_spec(spec)          # (the package's own __init__ is not executed)
    return importlib.import_module("ref_unimatch.attention"), importlib.import_module("ref_unimatch.utils")


def record(out, tag, module, inputs, result, gout):
    """Inputs, parameters, result and the gradients of (result * gout).sum()."""
    params = dict(module.named_parameters())
    grads = torch.autograd.grad(result, list(inputs.values()) + list(params.values()), gout)
    for i, (name, t) in enumerate(inputs.items()):
        out[tag + "in." + name] = t.detach().numpy()
        out[tag + "grad_in." + name] = grads[i].numpy()
    for i, (name, p) in enumerate(params.items()):
        out[tag + "param." + name] = p.detach().numpy()
        out[tag + "grad_param." + name] = grads[len(inputs) + i].numpy()
    out[tag + "out"] = result.detach().numpy()
    out[tag + "gout"] = gout.numpy()


def main():
    assert os.path.isdir(REF), "pass the root of the reference checkout"
    torch.set_default_dtype(torch.float64)
    att, utils = load_unimatch()
    env = load_classes(os.path.join(REF, "igs", "models", "unimatch", "transformer.py"), ["TransformerLayer"],
                       {"torch": torch, "nn": nn, "single_head_full_attention": att.single_head_full_attention,
                        "single_head_split_window_attention": att.single_head_split_window_attention})
    out = {}
    mask = utils.generate_shift_window_attn_mask((H, W), H // K, W // K, H // K // 2, W // K // 2, device=torch.device("cpu")).double()
    for no_ffn in (True, False):
        for shift in (False, True):
            seed = 10 * int(no_ffn) + int(shift)
            layer = TR.randomise(env["TransformerLayer"](d_model=DIM, nhead=1, no_ffn=no_ffn), seed)
            g = torch.Generator().manual_seed(100 + seed)
            source, target, gout = (torch.randn(B, H * W, DIM, generator=g) for _ in range(3))
            inputs = dict(source=source.requires_grad_(True), target=target.requires_grad_(True))
            result = layer(inputs["source"], inputs["target"], height=H, width=W, shifted_window_attn_mask=mask, attn_type="swin",
                           with_shift=shift, attn_num_splits=K)
            record(out, "layer_ffn%d_shift%d." % (int(not no_ffn), int(shift)), layer, inputs, result, gout)
    env = {"torch": torch, "nn": nn, "F": F, "maybe_allow_in_graph": lambda cls: cls,
           "Attention": lambda query_dim, **kw: TR.LinearAttention(query_dim)}
    env.update({n: getattr(typing, n) for n in ("Optional", "Dict", "Any", "Callable")})
    load_classes(os.path.join(REF, "igs", "models", "transformers.py"),
                 ["MemoryEfficientAttentionMixin", "GEGLU", "FeedForward", "BasicTransformerBlock"], env)
    block = TR.randomise(env["BasicTransformerBlock"](DIM, 2, 8), 7)
    g = torch.Generator().manual_seed(77)
    x, gout = torch.randn(2, 10, DIM, generator=g), torch.randn(2, 10, DIM, generator=g)
    inputs = dict(hidden_states=x.requires_grad_(True))
    record(out, "block.", block, inputs, block(inputs["hidden_states"]), gout)
    path = os.path.join(HERE, "ref_token_ops.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
