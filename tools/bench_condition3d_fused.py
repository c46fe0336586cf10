"""Timing of the fused condition3D forward (cond_fused.hip through igs_amd.motion.condition3d_fused, the weights packed once as
use_native_condition3d keeps them) against the three-step forward it replaces under no_grad (igs_amd.motion.condition3d: ray_condition ->
the PyTorch MLP -> modln), the same module on both sides, on the same GPU in the same process, alternating.  One JSON line per case and side:
{"case", "side": "fused" | "three_step", "B", "dtype", "ms": median of HIP-event-timed calls, "ms_min", "ms_max", "reps", "peak_mb"}.

  fwd        the forward under no_grad
  fwd_lift   the forward followed by grid_encoder_lift (8192 anchors), which reads either result in place
Shipped shape: V = 4, C = 128, hidden = 128, 128 x 128 maps, depth 1014 x 1352; B = 1 and 5; float32 features with the float32 MLP, and
float16 features under autocast (the fused side then runs its float16 instance, the three-step side a float16 MLP and modulation).
The last line states the gate: for float32, B = 1, forward, the fused median is below the three-step median and the min-max ranges do not
overlap; every other case is recorded as measured.

  --train    forward + backward instead: condition3d_fused_autograd (cond_fused_bwd.hip, the packs kept as the training binder keeps them)
             against condition3d forward + backward, the training path without it, with gradients to the features, the MLP's parameters
             and the LayerNorm's affine; N = 4 and N = 16 views, float32 and float16 features under autocast; case "fwd_bwd", sides
             "fused_autograd" | "three_step", "peak_mb" the rise of max_memory_allocated over one forward + backward.  The last line
             ("train_gate") states per dtype whether the native median is below the three-step median with disjoint min-max ranges at
             N = 16: the rule COND_FUSED_BWD_NATIVE follows.  With --out the lines replace the file's earlier fwd_bwd lines and leave
             the forward's lines as they are.

usage: python tools/bench_condition3d_fused.py [--reps 20] [--trace] [--train] [--out profiles/condition3d_fused_bench.jsonl]
  --trace: 3 calls per fused case and no timing (for a rocprofv3 --kernel-trace --stats run)
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

from bench_condition3d import peak, timed_pair  # noqa: E402


def train(args):
    import condition3d_restatement as CR
    from igs_amd import motion
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    V, C, H, W, Hd, Wd = 4, 128, 128, 128, 1014, 1352
    module = CR.AdaLNModule(C).to(dev)
    lines, verdicts = [], {}
    for B in (1, 4):
        N = B * V
        rays = torch.cat([torch.randn(B, V, H, W, 3, generator=g), torch.randn(B, V, H, W, 3, generator=g) * 1.7], -1).to(dev)
        depth = (1.0 + 5.0 * torch.rand(B, V, Hd, Wd, generator=g)).to(dev)
        gout = torch.randn(N, C, H, W, generator=g).to(dev)
        for dt in (torch.float32, torch.float16):
            x = torch.randn(N, C, H, W, generator=g).to(dt).to(dev).requires_grad_(True)
            cast = (lambda: torch.autocast("cuda", dtype=torch.float16)) if dt == torch.float16 else contextlib.nullcontext
            sides = dict(fused_autograd=lambda f, dt=dt: motion.condition3d_fused_autograd(f, rays, depth, module, mlp_dtype=dt),
                         three_step=lambda f: motion.condition3d(f, rays, depth, module))

            def make(side, x=x, cast=cast, sides=sides, gout=gout):
                fn = sides[side]

                def fwd_bwd():
                    x.grad = None
                    module.zero_grad(set_to_none=True)
                    with cast():
                        out = fn(x)
                    out.backward(gout)

                return fwd_bwd

            fa, fb = make("fused_autograd"), make("three_step")
            if args.trace:
                for _ in range(3):
                    fa()
                torch.cuda.synchronize()
                continue
            ra, rb = timed_pair(fa, fb, args.reps)
            case = dict(N=N, dtype=str(dt).replace("torch.", ""), C=C, H=H, W=W, case="fwd_bwd")
            for side, r, fn in (("fused_autograd", ra, fa), ("three_step", rb, fb)):
                lines.append(dict(case, side=side, ms=round(r[0], 4), ms_min=round(r[1], 4), ms_max=round(r[2], 4), reps=args.reps,
                                  peak_mb=round(peak(fn), 1)))
                print(json.dumps(lines[-1]), flush=True)
            if N == 16:
                verdicts[case["dtype"]] = dict(faster=bool(ra[0] < rb[0]), disjoint=bool(ra[2] < rb[1]), speedup=round(rb[0] / ra[0], 2),
                                               native=bool(ra[0] < rb[0] and ra[2] < rb[1]))
            del x
    if not args.trace:
        lines.append(dict(case="train_gate", N=16, verdicts=verdicts))
        print(json.dumps(lines[-1]), flush=True)
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        kept = []
        if os.path.exists(args.out):
            kept = [ln for ln in open(args.out).read().splitlines() if ln.strip() and json.loads(ln).get("case") not in ("fwd_bwd", "train_gate")]
        with open(args.out, "w") as f:
            for ln in kept:
                f.write(ln + "\n")
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_condition3d_fused needs a GPU"
    if args.train:
        return train(args)
    import condition3d_restatement as CR
    from igs_amd import motion
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    V, C, H, W, Hd, Wd, A = 4, 128, 128, 128, 1014, 1352, 8192
    module = CR.AdaLNModule(C).to(dev)
    packs = {dt: motion.pack_condition_mlp(module.mlp, dt) for dt in (torch.float32, torch.float16)}
    lines, verdicts = [], []
    for B in (1, 5):
        rays = torch.cat([torch.randn(B, V, H, W, 3, generator=g), torch.randn(B, V, H, W, 3, generator=g) * 1.7], -1).to(dev)
        depth = (1.0 + 5.0 * torch.rand(B, V, Hd, Wd, generator=g)).to(dev)
        pts = (torch.rand(B, A, 3, generator=g) * 2.0 - 1.0).to(dev)
        c2w = torch.eye(4).repeat(B, V, 1, 1)
        c2w[..., :3, 3] = torch.tensor([0.0, 0.0, -3.0]) + 0.3 * torch.randn(B, V, 3, generator=g)
        c2w = c2w.to(dev)
        fov = torch.tensor([[0.9, 0.9]], device=dev).repeat(B, 1)
        for dt in (torch.float32, torch.float16):
            x = torch.randn(B * V, C, H, W, generator=g).to(dt).to(dev)
            cast = (lambda: torch.autocast("cuda", dtype=torch.float16)) if dt == torch.float16 else contextlib.nullcontext
            sides = dict(fused=lambda f, dt=dt: motion.condition3d_fused(f, rays, depth, module, packed=packs[dt], mlp_dtype=dt),
                         three_step=lambda f: motion.condition3d(f, rays, depth, module))

            def make(side, case, x=x, cast=cast, sides=sides):
                fn = sides[side]

                def fwd():
                    with torch.no_grad(), cast():
                        return fn(x)

                def fwd_lift():
                    with torch.no_grad(), cast():
                        return motion.grid_encoder_lift(fn(x), pts, fov, c2w)

                return dict(fwd=fwd, fwd_lift=fwd_lift)[case]

            if args.trace:
                for fn in [make("fused", c) for c in ("fwd", "fwd_lift")]:
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                continue
            case = dict(B=B, dtype=str(dt).replace("torch.", ""), V=V, C=C, H=H, W=W)
            for name in ("fwd", "fwd_lift"):
                fa, fb = make("fused", name), make("three_step", name)
                ra, rb = timed_pair(fa, fb, args.reps)
                for side, r, fn in (("fused", ra, fa), ("three_step", rb, fb)):
                    lines.append(dict(case, case=name, side=side, ms=round(r[0], 4), ms_min=round(r[1], 4), ms_max=round(r[2], 4), reps=args.reps,
                                      peak_mb=round(peak(fn), 1)))
                    print(json.dumps(lines[-1]), flush=True)
                verdicts.append(dict(case=name, B=B, dtype=case["dtype"], faster=bool(ra[0] < rb[0]), disjoint=bool(ra[2] < rb[1]),
                                     speedup=round(rb[0] / ra[0], 2)))
            del x
    if not args.trace:
        gate = [v for v in verdicts if v["case"] == "fwd" and v["B"] == 1 and v["dtype"] == "float32"][0]
        lines.append(dict(case="gate", holds=bool(gate["faster"] and gate["disjoint"]), streaming=gate, cases=verdicts))
        print(json.dumps(lines[-1]), flush=True)
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        kept = []                                    # the --train lines of an earlier run stay
        if os.path.exists(args.out):
            kept = [ln for ln in open(args.out).read().splitlines() if ln.strip() and json.loads(ln).get("case") in ("fwd_bwd", "train_gate")]
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
            for ln in kept:
                f.write(ln + "\n")


if __name__ == "__main__":
    main()
