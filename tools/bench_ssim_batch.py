"""Timing of the batched SSIM / L1 of the AGM-Net training loss (ssim_batch.hip through igs_amd.losses) against the same lines in eager
PyTorch and against the single-image path on the same machine.  Prints one JSON line per case: {"case", "n", "ms": median over
HIP-event-timed calls, "ms_min", "ms_max", "reps", "peak_mb", "hbm_floor_ms"}.  The variants of one N are alternated call by call inside one
process, after a warm-up of every variant.

Images: [N, 3, 1014, 1352] (main.py:252-265: 4 examples x 8 views = 32 per step), N = 8 and 32; inputs as in tests/test_gpu_ssim_batch.py
(uniform gt, plus 0.15 * normal, clamped to [0, 1.2]).
  a ssim_native            mean, map = ssim(img1, img2); (0.2 * (1 - mean)).backward()
  b ssim_eager             the same lines on oracle.torch_losses.ssim_reference_call (the reference's five grouped 11 x 11 convolutions)
  c ssim_single_loop       a Python loop of the single-image path (ssim(x[n], gt[n:n+1], size_average=False)) over the N images, one
                           backward: what the package offered before the batched kernels
  d l1_ssim / l1_plus_ssim l1_ssim(pred, gt).loss.backward() against (l1_loss(pred, gt) + 0.2 * (1 - ssim(pred, gt)[0])).backward()
  e ssim_native_fwd        ssim(img1, img2) under no_grad
hbm_floor_ms: compulsory bytes per plane-pixel / 6.3 TB/s, every array read or written once:
  a 48 B = stats (x, y in; 3 derivative maps, SSIM map out) 24 + gradient (3 maps, x, y in; gradient out) 24;  d l1_ssim 44 B (no SSIM
  map), l1_plus_ssim 60 B (a, and l1_loss: x, y in, its gradient out);
  e 12 B = x, y in, SSIM map out.  (b and c carry a's floor for comparison.)
peak_mb: torch.cuda.max_memory_allocated() growth over one call, in MB.

Before timing, (a) is compared with (b) on the timed inputs at the bars of tests/test_gpu_ssim_batch.py: the mean within
1e-6 + 1e-5 |want|, every image's gradient with max error <= 2e-4 of its largest element and 99 % of the elements within 1e-3 relative;
the SSIM map of the first two images within 4 E32 + 1e-6 of oracle.torch_losses.ssim_map in float64 on the GPU, E32 = (b)'s own worst
error against that float64 run.  A disagreement ends the run with an error.

usage: python tools/bench_ssim_batch.py [--reps 20] [--n 8,32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_motion import peak  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
H, W, C = 1014, 1352, 3


def timed_alternating(fns, reps, warmup=3):
    """{name: (median, min, max) ms}: one HIP-event-timed call of every variant per round, `reps` rounds after `warmup` untimed ones."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ts.items()}


def compare(pred, gt):
    """(a) against (b), and the map against float64, at the tests' bars; raises on a disagreement."""
    import numpy as np
    from igs_amd.losses import ssim
    from oracle.torch_losses import ssim_map, ssim_reference_call
    n = pred.size(0)
    a = pred.clone().requires_grad_(True)
    mean, smap = ssim(a, gt)
    mean.backward()
    b = pred.clone().requires_grad_(True)
    want, want_map = ssim_reference_call(b, gt)
    want.backward()
    got, ref = mean.item(), want.item()
    if not abs(got - ref) <= 1e-6 + 1e-5 * abs(ref):
        raise SystemExit("bench_ssim_batch: mean SSIM %r against eager %r" % (got, ref))
    for i in range(n):
        x, y = a.grad[i].double().cpu().numpy(), b.grad[i].double().cpu().numpy()
        worst = np.abs(x - y).max()
        q99 = np.quantile(np.abs(x - y) / (np.abs(y) + 1e-3 * np.abs(y).max()), 0.99)
        if not (np.isfinite(x).all() and worst <= 2e-4 * np.abs(y).max() and q99 < 1e-3):
            raise SystemExit("bench_ssim_batch: gradient of image %d: max error %g of %g, 99 %% quantile %g" % (i, worst, np.abs(y).max(), q99))
    with torch.no_grad():
        m64 = ssim_map(pred[:2].double(), gt[:2].double())
        e32 = float((want_map[:2].double() - m64).abs().max())
        err = float((smap[:2].double() - m64).abs().max())
    if not err <= 4.0 * e32 + 1e-6:
        raise SystemExit("bench_ssim_batch: SSIM map error %g against float64, E32 %g" % (err, e32))
    return dict(mean=got, mean_eager=ref, map_err=err, e32=e32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", default="8,32")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ssim_batch needs a GPU"
    from igs_amd.losses import l1_loss, l1_ssim, ssim
    from oracle.torch_losses import ssim_reference_call
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for n in [int(s) for s in args.n.split(",")]:
        gt = torch.rand((n, C, H, W), generator=g).to(dev)
        pred = (gt + 0.15 * torch.randn((n, C, H, W), generator=g).to(dev)).clamp(0, 1.2).requires_grad_(True)
        print(json.dumps(dict(case="compare_native_with_eager", n=n, **compare(pred.detach(), gt))), flush=True)

        def backward(loss):
            pred.grad = None
            loss.backward()

        def native():
            backward(0.2 * (1.0 - ssim(pred, gt)[0]))

        def eager():
            backward(0.2 * (1.0 - ssim_reference_call(pred, gt)[0]))

        def single_loop():
            total = ssim(pred[0], gt[0:1], size_average=False)
            for i in range(1, n):
                total = total + ssim(pred[i], gt[i:i + 1], size_average=False)
            backward(0.2 * (1.0 - total / n).sum())

        def fused_loss():
            backward(l1_ssim(pred, gt).loss)

        def separate_loss():
            backward(l1_loss(pred, gt) + 0.2 * (1.0 - ssim(pred, gt)[0]))

        def native_fwd():
            with torch.no_grad():
                ssim(pred, gt)

        px = n * C * H * W
        floors = dict(ssim_native=48, ssim_eager=48, ssim_single_loop=48, l1_ssim=44, l1_plus_ssim=48 + 12, ssim_native_fwd=12)
        fns = dict(ssim_native=native, ssim_eager=eager, ssim_single_loop=single_loop, l1_ssim=fused_loss, l1_plus_ssim=separate_loss,
                   ssim_native_fwd=native_fwd)
        for k, (med, lo, hi) in timed_alternating(fns, args.reps).items():
            print(json.dumps(dict(case=k, n=n, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), reps=args.reps,
                                  peak_mb=round(peak(fns[k]), 1), hbm_floor_ms=round(px * floors[k] / HBM_BYTES_PER_S * 1e3, 4))), flush=True)
        pred.grad = None
        del pred, gt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
