"""Drop-in replacements for `igs/utils/loss_utils.py` (`l1_loss`, `ssim`) on the fused HIP kernels of loss_ops.hip and ssim_batch.hip.

The reference's SSIM runs five grouped 11x11 convolutions forward and their autograd graph backward: 7.3 ms per step at
1352x1014 on this GPU through PyTorch, against 0.08 ms for the two fused launches here.  `ssim` keeps the reference's signature and
serves two call shapes: the one the refine loop makes (`ssim(render, gt.unsqueeze(0), size_average=False)`, infer_batch.py:302) on the
single-image kernels, and the one the AGM-Net training loss makes (`ssim(img1, img2)` on `[N, C, H, W]` batches, main.py:252-265) on
the batched kernels; the gradient goes to the first image only and any other call shape raises.  `l1_ssim` is that training loss as
one call.  `depth_normal_loss` is RaDe-GS's regulariser (train.py:143-160) from one launch.  No PyTorch arithmetic on images and no CPU
path in this module (the restatements the kernels are checked against live in oracle/torch_losses.py).
"""
import collections

import torch

from . import _cabi


class _L1Mean(torch.autograd.Function):
    """mean |a - b| and d/da in ONE launch (igs_l1_mean_fwd_bwd through the compiled module: the value is finished on the device by the
    workgroup that ends last); backward is one scale of the stored sign / n map.  PyTorch's own sub / abs / mean take three launches
    forward and three backward."""

    @staticmethod
    def forward(ctx, a, b):
        out, grad = _cabi.ext().l1_mean(a, b)
        ctx.save_for_backward(grad)
        ctx.needs = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        ctx.shapes = (a.shape, b.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        ga = (g * grad).reshape(ctx.shapes[0]) if ctx.needs[0] else None
        gb = (-(g * grad)).reshape(ctx.shapes[1]) if ctx.needs[1] else None
        return ga, gb


def l1_loss(network_output, gt):
    """loss_utils.py:17-18 (`torch.abs(network_output - gt).mean()`).  Two float32 GPU tensors of the same shape go through the fused
    kernel; anything else is PyTorch's own three ops on the caller's tensors (no arithmetic of this package involved)."""
    if (network_output.is_cuda and gt.is_cuda and network_output.shape == gt.shape and network_output.dtype == torch.float32
            and gt.dtype == torch.float32 and network_output.numel() > 0):
        return _L1Mean.apply(network_output, gt)
    return torch.abs((network_output - gt)).mean()


class _FusedSsimMean(torch.autograd.Function):
    """mean SSIM(img1, img2) over all elements, finished on the device, and d/d img1 from the same two launches (igs_ssim_mean_fwd_bwd
    through the compiled module); backward is one scale of the stored map."""

    @staticmethod
    def forward(ctx, img1, img2):
        mean, grad = _cabi.ext().ssim_mean(img1, img2)
        ctx.save_for_backward(grad)
        ctx.in_shape = img1.shape
        return mean

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (g * grad).reshape(ctx.in_shape), None


class _SsimBatch(torch.autograd.Function):
    """Mean SSIM of every image of a [N, C, H, W] batch and d(mean_n)/d img1 from one call of igs_ssim_batch_fwd_bwd (three launches;
    two without a gradient, which then keeps nothing).  `per_image`: returns the [N] means; otherwise (mean of the means, SSIM map
    [N, C, H, W]), the map without a gradient.  Backward is one broadcast multiply of the stored map."""

    @staticmethod
    def forward(ctx, img1, img2, per_image, want_grad):
        n = img1.size(0)
        means, _, grad, ssim_map = _cabi.ext()._loss.ssim_batch(img1, img2, 1.0, 0.0, want_grad, not per_image, False)
        if want_grad:
            ctx.save_for_backward(grad)
        ctx.per_image, ctx.in_shape = per_image, img1.shape
        if per_image:
            return means[:n]
        ctx.mark_non_differentiable(ssim_map)
        return means[n], ssim_map

    @staticmethod
    def backward(ctx, g, *_):
        (grad,) = ctx.saved_tensors
        n = ctx.in_shape[0]
        scale = g.reshape(n, 1, 1, 1) if ctx.per_image else g / n
        return (grad * scale).reshape(ctx.in_shape), None, None, None


def _wants_grad(t):
    """Whether a backward can reach `t` from this call (inside Function.forward `needs_input_grad` is set under no_grad too)."""
    return torch.is_grad_enabled() and t.requires_grad


def _batch_call(img1, img2):
    """The AGM-Net call shape (main.py:254-257): two float32 GPU batches [N, C, H, W] of one shape, the second without a gradient."""
    return (img1.dim() == 4 and img2.dim() == 4 and img1.shape == img2.shape and img1.numel() > 0 and img1.is_cuda and img2.is_cuda
            and img1.dtype == torch.float32 and img2.dtype == torch.float32 and not img2.requires_grad)


def ssim(img1, img2, window_size=11, size_average=True):
    """loss_utils.py:34-63, served by the fused HIP kernels for GPU tensors and the 11x11 window, gradient w.r.t. img1 only:
      - the call the refine loop makes: one image ([3,H,W] or [1,3,H,W] on either side), `size_average=False` -> the mean, shape [1];
      - the call the training loss makes: two float32 batches [N,C,H,W] of one shape.  `size_average=True` -> `(mean, ssim_map)` as the
        reference (mean 0-dim: the mean of the per-image means, which all weigh the same; ssim_map [N,C,H,W]); `size_average=False`
        with N > 1 -> the per-image means [N].  Unlike the reference's, the returned map carries NO gradient (main.py never
        differentiates it).
    Any other call shape or dtype raises NotImplementedError: there is no PyTorch / CPU fallback in this package."""
    single = all(t.dim() == 3 or (t.dim() == 4 and t.size(0) == 1) for t in (img1, img2))
    if (img1.is_cuda and img2.is_cuda and window_size == 11 and not size_average and single and not img2.requires_grad
            and img1.shape[-3:] == img2.shape[-3:]):
        return _FusedSsimMean.apply(img1, img2).reshape(1)
    if window_size == 11 and _batch_call(img1, img2) and (size_average or img1.size(0) > 1):
        return _SsimBatch.apply(img1, img2, not size_average, _wants_grad(img1))
    raise NotImplementedError("igs_amd.losses.ssim serves ssim(render, gt.unsqueeze(0), size_average=False) (infer_batch.py:302) and "
                              "ssim(img1, img2) on two float32 [N, C, H, W] batches of one shape (main.py:257), on GPU tensors with the "
                              "11x11 window and no gradient to img2; other call shapes and dtypes are not implemented (no CPU / "
                              "PyTorch fallback)")


L1Ssim = collections.namedtuple("L1Ssim", ["loss", "l1", "ssim"])


class _L1SsimBatch(torch.autograd.Function):
    """(mean L1, mean SSIM, d/d pred of lambda_l1 * mean L1 - lambda_ssim * mean SSIM) of a [N, C, H, W] batch from ONE call of
    igs_ssim_batch_fwd_bwd: c_ssim = -lambda_ssim / N, c_l1 = lambda_l1 / N.  The loss is combined from the two device means."""

    @staticmethod
    def forward(ctx, pred, gt, lambda_ssim, lambda_l1, want_grad):
        n = pred.size(0)
        means, l1_means, grad, _ = _cabi.ext()._loss.ssim_batch(pred, gt, -lambda_ssim / n, lambda_l1 / n, want_grad, False, True)
        if want_grad:
            ctx.save_for_backward(grad)
        ctx.in_shape = pred.shape
        l1, s = l1_means[n], means[n]
        ctx.mark_non_differentiable(l1, s)
        return lambda_l1 * l1 + lambda_ssim * (1.0 - s), l1, s

    @staticmethod
    def backward(ctx, g, *_):
        (grad,) = ctx.saved_tensors
        return (grad * g).reshape(ctx.in_shape), None, None, None, None


def l1_ssim(pred, gt, lambda_ssim=0.2, lambda_l1=1.0):
    """The AGM-Net training loss (main.py:252-265 with lambda_lpips = 0) as one native call:
        loss = lambda_l1 * mean|pred - gt| + lambda_ssim * (1 - mean SSIM(pred, gt)),   autograd to `pred` only.
    pred, gt: float32 GPU tensors [..., C, H, W] of one shape (the leading dimensions are flattened into the batch, as main.py's
    rearrange does).  Returns the named tuple (loss, l1, ssim) of 0-dim tensors; l1 and ssim are detached (main.py:255,264 log them).
    Nothing is read back to the host."""
    if pred.dim() < 3 or pred.shape != gt.shape:
        raise NotImplementedError("igs_amd.losses.l1_ssim: pred and gt must share one shape [..., C, H, W]")
    a, b = pred.reshape((-1,) + tuple(pred.shape[-3:])), gt.reshape((-1,) + tuple(gt.shape[-3:]))
    if not _batch_call(a, b):
        raise NotImplementedError("igs_amd.losses.l1_ssim serves non-empty float32 GPU tensors and no gradient to gt (no CPU / PyTorch "
                                  "fallback)")
    return L1Ssim(*_L1SsimBatch.apply(a, b, float(lambda_ssim), float(lambda_l1), _wants_grad(a)))


class _DepthNormalLoss(torch.autograd.Function):
    """RaDe-GS depth-normal consistency (train.py:143-160, graphics_utils.py:97-126): value and the three gradient maps from ONE
    launch (igs_depth_normal_loss_fwd_bwd); backward scales the stored maps by the upstream gradient."""

    @staticmethod
    def forward(ctx, depth, mdepth, normal, tan_fovx, tan_fovy, depth_ratio):
        L = _cabi.lib()
        dev = depth.device
        H, W = int(normal.shape[-2]), int(normal.shape[-1])
        d, m, n = depth.contiguous().float(), mdepth.contiguous().float(), normal.contiguous().float()
        gd, gm, gn = torch.empty_like(d), torch.empty_like(m), torch.empty_like(n)
        shards = torch.empty(1024, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = L.igs_depth_normal_loss_fwd_bwd(torch.cuda.current_stream(dev).cuda_stream, W, H, float(tan_fovx), float(tan_fovy),
                                                 d.data_ptr(), m.data_ptr(), n.data_ptr(), 1.0, float(depth_ratio), gd.data_ptr(),
                                                 gm.data_ptr(), gn.data_ptr(), shards.data_ptr())
        if rc != 0:
            raise RuntimeError("igs_depth_normal_loss_fwd_bwd failed: %d" % rc)
        ctx.save_for_backward(gd, gm, gn)
        ctx.shapes = (depth.shape, mdepth.shape, normal.shape)
        return shards[::16].sum()

    @staticmethod
    def backward(ctx, g):
        gd, gm, gn = ctx.saved_tensors
        sd, sm, sn = ctx.shapes
        return (g * gd).reshape(sd), (g * gm).reshape(sm), (g * gn).reshape(sn), None, None, None


def depth_normal_loss(pkg, cam, depth_ratio=0.6):
    """`(1 - depth_ratio) * mean(1 - n . n(depth)) + depth_ratio * mean(1 - n . n(mdepth))` on the rasterizer's outputs
    (`pkg`: depth_pred, mdepth, normal), differentiable w.r.t. all three; GPU tensors only."""
    if not pkg["normal"].is_cuda:
        raise RuntimeError("igs_amd.losses.depth_normal_loss: tensors must be on a GPU (no CPU fallback)")
    return _DepthNormalLoss.apply(pkg["depth_pred"], pkg["mdepth"], pkg["normal"], cam.tanfovx, cam.tanfovy, depth_ratio)
