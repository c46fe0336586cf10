"""Writes tests/golden/ref_ssim_batch.npz: the reference's own `ssim` on a BATCH of images, the call shape of the AGM-Net training loss
(main.py:252-265).  Run once on the CPU next to a checkout of the reference; the tests read only the .npz.

Produced by submodules/RaDe-GS/utils/loss_utils.py (loaded the way make_golden.py loads it), which holds the same `ssim` as
igs/utils/loss_utils.py:33-63 up to the return statement: with size_average=True the RaDe-GS file returns `ssim_map.mean()`, the IGS file
`(ssim_map.mean(), ssim_map)` (that one needs `icecream` to import).  Contents, for a seeded [3, 3, 20, 27] batch:
  x, gt              the inputs (gt uniform, x = clamp(gt + 0.15 normal, 0, 1.2))
  mean, mean_grad    ssim(x, gt) and its autograd gradient w.r.t. x
  per_image          ssim(x, gt, size_average=False), shape [3]
  per_image_w, per_image_grad   the weights w and the gradient of (w * per_image).sum() w.r.t. x
"""
import importlib.util
import os

import numpy as np
import torch

RADE = "/root/reference/submodules/RaDe-GS/utils"
HERE = os.path.dirname(os.path.abspath(__file__))


def load_rade(name):
    spec = importlib.util.spec_from_file_location("rade_" + name, os.path.join(RADE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    lu = load_rade("loss_utils")
    g = torch.Generator().manual_seed(20261019)
    gt = torch.rand((3, 3, 20, 27), generator=g)
    x = (gt + 0.15 * torch.randn(gt.shape, generator=g)).clamp(0, 1.2)
    a = x.clone().requires_grad_(True)
    mean = lu.ssim(a, gt)
    (mean_grad,) = torch.autograd.grad(mean, a)
    b = x.clone().requires_grad_(True)
    per_image = lu.ssim(b, gt, size_average=False)
    w = torch.tensor([1.0, 0.5, -2.5])
    (per_image_grad,) = torch.autograd.grad((w * per_image).sum(), b)
    out = dict(x=x.numpy(), gt=gt.numpy(), mean=mean.detach().numpy(), mean_grad=mean_grad.numpy(), per_image=per_image.detach().numpy(),
               per_image_w=w.numpy(), per_image_grad=per_image_grad.numpy())
    np.savez(os.path.join(HERE, "ref_ssim_batch.npz"), **out)
    print("wrote ref_ssim_batch.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
