"""Timing of the fused 2x bilinear upsample + 3x3 convolution (upconv.hip through igs_amd.motion.upsample_conv, the weights packed once
as the module cache keeps them) against the eager two lines it replaces under no_grad (F.interpolate -> nn.Conv2d, igs/IGS.py:133-134),
the same module on both sides, on the same GPU in the same process, alternating.  One JSON line per case and side:
{"case", "side": "native" | "eager", "N", "dtype", "ms": median of HIP-event-timed calls, "ms_min", "ms_max", "reps", "peak_mb"}.

  fwd        the step under no_grad
  fwd_cond   the step followed by condition3d_fused, which reads either result in place (one pair: N = 4, float32)
Shipped shape: 128 -> 128 channels, 64 x 64 -> 128 x 128; N = 4 (one streamed frame's views) and 20; float32, and float32 features under
autocast to float16 (the native side then runs its float16 instance, the eager side MIOpen's half convolution).
"kernel" lines: the native call issued 10 times back to back between one pair of events, per call, so that the launch overhead of a
single call is hidden; for float32 also as a fraction of the 0.123 ms matrix floor per 4 images (19.3 GFLOP at 157 TFLOP/s).
The last line sums up, per dtype and N, which side was faster and whether the min-max ranges are disjoint: UPCONV_NATIVE follows it.

--train times the training step instead (igs_amd.motion.upsample_conv_autograd over upconv.hip and upconv_bwd.hip against the eager two
lines with autograd, the parent's training path): forward + backward with gradients to x, weight and bias, N = 4 and 32, float32 and
float32 tensors under autocast to float16.  The weights change every step, so each timed call first bumps weight's version in place (both
sides) and the native side repacks its three packs.  Lines {"case": "train", ...} as above, then "bwd_kernel" lines: igs_upconv_bwd alone,
dx only (dgrad) and dW + db only (wgrad + reduce), 10 calls back to back, for float32 with the 157 TFLOP/s matrix floor (dgrad's includes
its 1.42 x halo recomputation) and the fraction reached.  The summary line is what UPCONV_BWD_NATIVE follows.  With --train, --out appends.

usage: python tools/bench_upconv.py [--reps 20] [--trace] [--train] [--out profiles/upconv_bench.jsonl]
  --trace: 3 calls per native case and no timing (for a rocprofv3 --kernel-trace --stats run)
"""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_condition3d import peak, timed_pair  # noqa: E402

FLOOR_MS_PER_IMAGE = 2 * 9 * 128 * 128 * 128 * 128 / 157e12 * 1e3           # float32 matrix path, one 128 x 128 image


def back_to_back(fn, calls=10, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / calls)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


DGRAD_RECOMPUTE = (8 * 32) / (6 * 30)                                        # dup pixels computed per dup pixel needed: 3 x 15 tiles


def train(args):
    from igs_amd import motion
    from igs_amd._cabi import ext
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    C, H, W = 128, 64, 64
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(C, C, 3, stride=1, padding=1).to(dev)
    lines, verdicts = [], []
    for N in (4, 32):
        x = torch.randn(N, C, H, W, generator=g).to(dev).requires_grad_(True)
        for dt in (torch.float32, torch.float16):
            cast = (lambda: torch.autocast("cuda", dtype=torch.float16)) if dt == torch.float16 else contextlib.nullcontext
            gout = torch.randn(N, C, 2 * H, 2 * W, generator=g).to(dev).to(dt)
            sides = dict(native=lambda f, dt=dt: motion.upsample_conv_autograd(f, conv, conv_dtype=dt),
                         eager=lambda f: conv(F.interpolate(f, scale_factor=2, mode="bilinear", align_corners=False)))

            def make(side, x=x, cast=cast, sides=sides, gout=gout):
                fn = sides[side]

                def step():
                    with torch.no_grad():
                        conv.weight.add_(0.0)                    # an optimiser step: the version moves, the native side repacks
                    x.grad = conv.weight.grad = conv.bias.grad = None
                    with cast():
                        out = fn(x)
                    out.backward(gout)
                    return x.grad

                return step

            case = dict(N=N, dtype=str(dt).replace("torch.", ""), C=C, H=H, W=W)
            fa, fb = make("native"), make("eager")
            if args.trace:
                for _ in range(3):
                    fa()
                torch.cuda.synchronize()
                continue
            ra, rb = timed_pair(fa, fb, args.reps)
            for side, r, fn in (("native", ra, fa), ("eager", rb, fb)):
                lines.append(dict(case, case="train", side=side, ms=round(r[0], 4), ms_min=round(r[1], 4), ms_max=round(r[2], 4), reps=args.reps,
                                  peak_mb=round(peak(fn), 1)))
                print(json.dumps(lines[-1]), flush=True)
            verdicts.append(dict(case="train", N=N, dtype=case["dtype"], native_faster=bool(ra[0] < rb[0]),
                                 disjoint=bool(ra[2] < rb[1] or rb[2] < ra[1]), speedup=round(rb[0] / ra[0], 2)))
            wt = motion.pack_upsample_conv(conv, dt, transposed=True)[2]
            xd = x.detach()
            for part, want, scale in (("dgrad", (True, False, False), DGRAD_RECOMPUTE), ("wgrad", (False, True, True), 1.0)):
                k = back_to_back(lambda: ext()._upconv.upconv_bwd(xd, wt, gout, *want))
                ln = dict(case, case="bwd_kernel", side=part, ms=round(k[0], 4), ms_min=round(k[1], 4), ms_max=round(k[2], 4), calls=10, reps=5)
                if dt == torch.float32:
                    ln["floor_ms"] = round(FLOOR_MS_PER_IMAGE * N * scale, 4)
                    ln["floor_fraction"] = round(FLOOR_MS_PER_IMAGE * N * scale / k[0], 3)
                lines.append(ln)
                print(json.dumps(ln), flush=True)
            del gout
        del x
    if not args.trace:
        lines.append(dict(case="train_summary", cases=verdicts))
        print(json.dumps(lines[-1]), flush=True)
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_upconv needs a GPU"
    if args.train:
        return train(args)
    import condition3d_restatement as CR
    from igs_amd import motion
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    C, H, W, Hd, Wd = 128, 64, 64, 1014, 1352
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(C, C, 3, stride=1, padding=1).to(dev).requires_grad_(False)
    module = CR.AdaLNModule(C).to(dev)
    packs = {dt: motion.pack_upsample_conv(conv, dt) for dt in (torch.float32, torch.float16)}
    cpack = motion.pack_condition_mlp(module.mlp, torch.float32)
    lines, verdicts = [], []
    for N in (4, 20):
        x = torch.randn(N, C, H, W, generator=g).to(dev)
        rays = torch.cat([torch.randn(N // 4, 4, 2 * H, 2 * W, 3, generator=g), torch.randn(N // 4, 4, 2 * H, 2 * W, 3, generator=g) * 1.7], -1).to(dev)
        depth = (1.0 + 5.0 * torch.rand(N // 4, 4, Hd, Wd, generator=g)).to(dev)
        for dt in (torch.float32, torch.float16):
            cast = (lambda: torch.autocast("cuda", dtype=torch.float16)) if dt == torch.float16 else contextlib.nullcontext
            sides = dict(native=lambda f, dt=dt: motion.upsample_conv(f, conv, packed=packs[dt], conv_dtype=dt),
                         eager=lambda f: conv(F.interpolate(f, scale_factor=2, mode="bilinear", align_corners=False)))

            def make(side, case, x=x, cast=cast, sides=sides, rays=rays, depth=depth):
                fn = sides[side]

                def fwd():
                    with torch.no_grad(), cast():
                        return fn(x)

                def fwd_cond():
                    with torch.no_grad(), cast():
                        return motion.condition3d_fused(fn(x), rays, depth, module, packed=cpack, mlp_dtype=torch.float32)

                return dict(fwd=fwd, fwd_cond=fwd_cond)[case]

            names = ("fwd", "fwd_cond") if (N == 4 and dt == torch.float32) else ("fwd",)
            if args.trace:
                for fn in [make("native", c) for c in names]:
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                continue
            case = dict(N=N, dtype=str(dt).replace("torch.", ""), C=C, H=H, W=W)
            for name in names:
                fa, fb = make("native", name), make("eager", name)
                ra, rb = timed_pair(fa, fb, args.reps)
                for side, r, fn in (("native", ra, fa), ("eager", rb, fb)):
                    lines.append(dict(case, case=name, side=side, ms=round(r[0], 4), ms_min=round(r[1], 4), ms_max=round(r[2], 4), reps=args.reps,
                                      peak_mb=round(peak(fn), 1)))
                    print(json.dumps(lines[-1]), flush=True)
                verdicts.append(dict(case=name, N=N, dtype=case["dtype"], native_faster=bool(ra[0] < rb[0]),
                                     disjoint=bool(ra[2] < rb[1] or rb[2] < ra[1]), speedup=round(rb[0] / ra[0], 2)))
            for side in ("native", "eager"):
                k = back_to_back(make(side, "fwd"))
                ln = dict(case, case="kernel", side=side, ms=round(k[0], 4), ms_min=round(k[1], 4), ms_max=round(k[2], 4), calls=10, reps=5)
                if dt == torch.float32:
                    ln["floor_ms"] = round(FLOOR_MS_PER_IMAGE * N, 4)
                    ln["floor_fraction"] = round(FLOOR_MS_PER_IMAGE * N / k[0], 3)
                lines.append(ln)
                print(json.dumps(ln), flush=True)
        del x, rays, depth
    if not args.trace:
        lines.append(dict(case="summary", cases=verdicts))
        print(json.dumps(lines[-1]), flush=True)
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
