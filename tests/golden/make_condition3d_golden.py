"""Generates tests/golden/ref_condition3d.npz: outputs of the reference's own ray_to_plucker, rsh_cart_3, ModLN and IGS.condition3D
(igs/IGS.py), data only.

Run in the build container only (needs the reference checkout and einops):
    python tests/golden/make_condition3d_golden.py REFERENCE_ROOT        (or IGS_REFERENCE in the environment)
igs/IGS.py does not import here, so only the AST nodes of the two functions, the ModLN class and the condition3D method are compiled; the
reference is read at run time and none of its text is stored.  A SimpleNamespace with cfg.local_ray = False and a ModLN(8, 33, 1e-6) serves
as `self`.  Case: B = 2, V = 2, C = 8, a non-square 6 x 10 map, depth 15 x 23 (a non-integer scale), ray directions that are NOT unit
vectors, norm.weight / norm.bias randomised away from 1 / 0, x = 3 + 0.5 randn (a non-zero pixel mean).  Stored: the inputs, all module
parameters, cond, mod, out, and for a fixed upstream gradient the autograd gradients to x, norm.weight, norm.bias and the MLP's output.

Before the file is written the reference's float32 outputs and gradients are checked against the float64 restatements within the derived
bounds of tests/condition3d_restatement.py.
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import condition3d_restatement as CR  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IGS_REFERENCE", "")


def load_nodes(path, env):
    """Compiles ray_to_plucker, rsh_cart_3, class ModLN and the method IGS.condition3D (as a plain function) into env."""
    tree = ast.parse(open(path).read())
    body = []
    for n in tree.body:
        if isinstance(n, ast.FunctionDef) and n.name in ("ray_to_plucker", "rsh_cart_3"):
            for a in n.args.args:
                a.annotation = None
            n.returns = None
            body.append(n)
        elif isinstance(n, ast.ClassDef) and n.name == "ModLN":
            body.append(n)
        elif isinstance(n, ast.ClassDef):
            body += [m for m in n.body if isinstance(m, ast.FunctionDef) and m.name == "condition3D"]
    assert len(body) == 4, [getattr(b, "name", None) for b in body]
    exec(compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), path, "exec"), env)
    return env


def within(name, got, want, bound):
    err = (got.double() - want).abs()
    ratio = (err / bound).max().item()
    print("%-12s max |reference - restatement| = %.3e, max |value| = %.3e, largest error / bound = %.3f" % (name, err.max().item(), want.abs().max().item(), ratio))
    assert (err <= bound).all(), name


def main():
    assert os.path.isdir(REF), "pass the root of the reference checkout"
    from einops import rearrange
    env = load_nodes(os.path.join(REF, "igs", "IGS.py"), {"torch": torch, "nn": nn, "F": F, "rearrange": rearrange})
    g = torch.Generator().manual_seed(20251)
    B, V, C, H, W, Hd, Wd = 2, 2, 8, 6, 10, 15, 23
    module = env["ModLN"](C, 33, 1e-6)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
        module.norm.weight.copy_(1.0 + 0.5 * torch.randn(C, generator=g))
        module.norm.bias.copy_(0.4 * torch.randn(C, generator=g))
    self = types.SimpleNamespace(cfg=types.SimpleNamespace(local_ray=False), ModLN=module)
    x = (3.0 + 0.5 * torch.randn(B * V, C, H, W, generator=g)).requires_grad_(True)
    rays = torch.cat([torch.randn(B, V, H, W, 3, generator=g) * 1.5,
                      torch.randn(B, V, H, W, 3, generator=g) * (0.5 + 2.0 * torch.rand(B, V, H, W, 1, generator=g))], -1)
    depth = 1.0 + 5.0 * torch.rand(B, V, Hd, Wd, generator=g)
    # the pieces on their own
    pl = env["ray_to_plucker"](rays)
    cond = torch.cat([env["rsh_cart_3"](pl[..., :3]), env["rsh_cart_3"](pl[..., 3:6]),
                      F.interpolate(depth.reshape(B * V, 1, Hd, Wd), size=(H, W), mode="bilinear", align_corners=False).squeeze(1)
                      .reshape(B, V, H, W, 1)], -1).reshape(B * V, H, W, 33)
    kept = {}

    def keep(_module, _inputs, output):
        kept["mod"] = output
        output.retain_grad()

    handle = module.mlp.register_forward_hook(keep)
    out = env["condition3D"](self, x, rays, depth)
    handle.remove()
    assert out.shape == (B * V, C, H, W) and out.stride() == (C * H * W, 1, W * C, C)           # the channels-last-strided view
    gout = torch.randn(B * V, C, H, W, generator=g)
    out.backward(gout)
    mod = kept["mod"]
    w, b = module.norm.weight, module.norm.bias
    # the reference's float32 results within the derived bounds of the float64 restatements
    within("cond", cond, CR.ray_condition_restate(rays.double(), depth.double()), CR.ray_condition_bound(rays, depth))
    xd, md, wd, bd = x.detach().double(), mod.detach().double(), w.detach().double(), b.detach().double()
    within("out", out.detach(), CR.modln_restate(xd, md, wd, bd, 1e-6), CR.modln_forward_bound(x.detach(), mod.detach(), w.detach(), b.detach(), 1e-6))
    dx, dmod, dw, db = CR.modln_backward_restate(xd, md, wd, bd, 1e-6, gout.double())
    bb = CR.modln_backward_bounds(x.detach(), mod.detach(), w.detach(), b.detach(), 1e-6, gout)
    within("d x", x.grad, dx, bb["dx"])
    within("d mod", mod.grad, dmod, bb["dmod"])
    within("d weight", w.grad, dw, bb["dweight"])
    within("d bias", b.grad, db, bb["dbias"])
    arrays = dict(x=x.detach(), rays=rays, depth=depth, cond=cond, mod=mod.detach(), out=out.detach().contiguous(), gout=gout,
                  dx=x.grad, dmod=mod.grad, dweight=w.grad, dbias=b.grad, norm_weight=w.detach(), norm_bias=b.detach(),
                  mlp0_weight=module.mlp[0].weight.detach(), mlp0_bias=module.mlp[0].bias.detach(),
                  mlp2_weight=module.mlp[2].weight.detach(), mlp2_bias=module.mlp[2].bias.detach(), eps=torch.tensor(1e-6, dtype=torch.float64),
                  out_strides=torch.tensor(out.stride()))
    path = os.path.join(HERE, "ref_condition3d.npz")
    np.savez_compressed(path, **{k: v.numpy() for k, v in arrays.items()})
    print("ref_condition3d.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
