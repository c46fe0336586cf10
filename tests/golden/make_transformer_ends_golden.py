"""Generates tests/golden/ref_transformer_ends.npz: outputs and autograd gradients of the reference's own Transformer1D
(igs/models/transformers.py) around its BasicTransformerBlock, data only.

Run in the build container only (needs the reference checkout):  python tests/golden/make_transformer_ends_golden.py REFERENCE_ROOT   (or IGS_REFERENCE in the environment)
The file does not import here (diffusers, the igs package), so only the AST nodes of the classes MemoryEfficientAttentionMixin, GEGLU,
FeedForward, BasicTransformerBlock and Transformer1D are compiled, as make_token_ops_golden.py does; the reference is read at run time and
none of its text is stored.  BaseModule is a stand-in whose __init__(cfg) builds self.Config(**cfg) and calls configure();
maybe_allow_in_graph is the identity; diffusers' Attention is the one-Linear stand-in of tests/token_ops_restatement.py: the file pins the
wiring around the blocks, not the attention.

Cases, float64, B = 2: (in_channels 12, norm_num_groups 3, A 7, num_layers 0) and (16, 4, 10, 1) with two heads of 8; every Linear and
LayerNorm randomised by token_ops_restatement.randomise, the GroupNorm's weight and bias away from 1 / 0.  Stored per case: the input,
every parameter under its state_dict() key, the output, and autograd's gradients to the input and to every parameter for a fixed upstream
gradient.
"""
import os
import sys
import typing
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import token_ops_restatement as TR  # noqa: E402
import transformer_ends_restatement as ER  # noqa: E402
from make_token_ops_golden import load_classes, record  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IGS_REFERENCE", "")
CASES = [dict(in_channels=12, norm_num_groups=3, A=7, num_layers=0), dict(in_channels=16, norm_num_groups=4, A=10, num_layers=1)]
BATCH, HEADS, HEAD_DIM = 2, 2, 8


class BaseModule(nn.Module):
    @dataclass
    class Config:
        pass

    def __init__(self, cfg=None):
        super().__init__()
        self.cfg = self.Config(**(cfg or {}))
        self.configure()

    def configure(self):
        pass


def main():
    assert os.path.isdir(REF), "pass the root of the reference checkout"
    torch.set_default_dtype(torch.float64)
    env = {"torch": torch, "nn": nn, "F": F, "maybe_allow_in_graph": lambda cls: cls, "dataclass": dataclass, "field": field,
           "BaseModule": BaseModule, "Attention": lambda query_dim, **kw: TR.LinearAttention(query_dim)}
    env.update({n: getattr(typing, n) for n in ("Optional", "Dict", "Any", "Callable")})
    load_classes(os.path.join(REF, "igs", "models", "transformers.py"),
                 ["MemoryEfficientAttentionMixin", "GEGLU", "FeedForward", "BasicTransformerBlock", "Transformer1D"], env)
    out = {}
    for i, case in enumerate(CASES):
        model = ER.randomise(env["Transformer1D"](dict(num_attention_heads=HEADS, attention_head_dim=HEAD_DIM, in_channels=case["in_channels"],
                                                       norm_num_groups=case["norm_num_groups"], num_layers=case["num_layers"])), 20 + i)
        assert model.norm.eps == 1e-6
        g = torch.Generator().manual_seed(200 + i)
        x = 2.0 * torch.randn(BATCH, case["in_channels"], case["A"], generator=g) + 0.5
        gout = torch.randn(BATCH, case["in_channels"], case["A"], generator=g)
        inputs = dict(hidden_states=x.requires_grad_(True))
        record(out, "case%d." % i, model, inputs, model(inputs["hidden_states"]), gout)
    path = os.path.join(HERE, "ref_transformer_ends.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
