"""Timing of the native condition3D (cond.hip through igs_amd.motion.condition3d) against the reference's composition restated call
for call in PyTorch (tests/condition3d_restatement.reference_composition), the same module weights on both sides, on the same GPU in the
same process, alternating.  One JSON line per case and side:
{"case", "side": "native" | "reference", "B", "dtype", "ms": median of HIP-event-timed calls, "ms_min", "ms_max", "reps", "peak_mb"}.

  fwd            (a) forward under no_grad
  fwd_bwd        (b) forward + backward to the features and all parameters (LayerNorm's affine and the MLP)
  fwd_lift       (c) (a) followed by grid_encoder_lift: the reference hands the lift a channels-last-strided view (the lift copies it),
  fwd_bwd_lift       the native result is read in place; and (b) through the lift
  modln_fwd / modln_bwd   the fused kernel alone (native only), with algo_mb = its unavoidable bytes and algo_tbs = bytes / median time
Shipped shape: V = 4, C = 128, 128 x 128 maps, depth 1014 x 1352, A = 8192 anchors; B = 1 and 5; float32 features, and float16 features
under autocast (what makes the reference's LayerNorm run at all on half inputs; the MLP then emits a float16 modulation on both sides).
The last line states the merge condition: for every case the native median is below the reference's and the min-max ranges do not overlap.

usage: python tools/bench_condition3d.py [--reps 20] [--trace] [--out profiles/condition3d_bench.jsonl]
  --trace: 3 calls per native case and no timing (for a rocprofv3 --kernel-trace --stats run)
"""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def timed_pair(fa, fb, reps, warmup=3):
    """Medians (and min / max) of fa and fb, timed alternately."""
    for _ in range(warmup):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
    ta.sort(); tb.sort()
    return (ta[len(ta) // 2], ta[0], ta[-1]), (tb[len(tb) // 2], tb[0], tb[-1])


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_condition3d needs a GPU"
    import condition3d_restatement as CR
    from igs_amd import motion
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    V, C, H, W, Hd, Wd, A = 4, 128, 128, 128, 1014, 1352, 8192
    module = CR.AdaLNModule(C).to(dev)
    params = list(module.parameters())
    lines, verdicts = [], []
    for B in (1, 5):
        rays = torch.cat([torch.randn(B, V, H, W, 3, generator=g), torch.randn(B, V, H, W, 3, generator=g) * 1.7], -1).to(dev)
        depth = (1.0 + 5.0 * torch.rand(B, V, Hd, Wd, generator=g)).to(dev)
        pts = (torch.rand(B, A, 3, generator=g) * 2.0 - 1.0).to(dev)
        c2w = torch.eye(4).repeat(B, V, 1, 1)
        c2w[..., :3, 3] = torch.tensor([0.0, 0.0, -3.0]) + 0.3 * torch.randn(B, V, 3, generator=g)
        c2w = c2w.to(dev)
        fov = torch.tensor([[0.9, 0.9]], device=dev).repeat(B, 1)
        gout = torch.randn(B * V, C, H, W, generator=g).to(dev)
        glift = torch.randn(B, A, C, generator=g).to(dev)
        for dt in (torch.float32, torch.float16):
            x = torch.randn(B * V, C, H, W, generator=g).to(dt).to(dev)
            xg = x.clone().requires_grad_(True)
            cast = (lambda: torch.autocast("cuda", dtype=torch.float16)) if dt == torch.float16 else contextlib.nullcontext
            sides = dict(native=lambda f: motion.condition3d(f, rays, depth, module),
                         reference=lambda f: CR.reference_composition(f, rays, depth, module))

            def make(side, case):
                fn = sides[side]

                def fwd():
                    with torch.no_grad(), cast():
                        return fn(x)

                def fwd_bwd():
                    with cast():
                        out = fn(xg)
                    return torch.autograd.grad(out, [xg] + params, gout)

                def fwd_lift():
                    with torch.no_grad(), cast():
                        return motion.grid_encoder_lift(fn(x), pts, fov, c2w)

                def fwd_bwd_lift():
                    with cast():
                        out = motion.grid_encoder_lift(fn(xg), pts, fov, c2w)
                    return torch.autograd.grad(out, [xg] + params, glift)

                return dict(fwd=fwd, fwd_bwd=fwd_bwd, fwd_lift=fwd_lift, fwd_bwd_lift=fwd_bwd_lift)[case]

            # the fused kernel alone
            with torch.no_grad(), cast():
                mod = module.mlp(motion.ray_condition(rays, depth, (H, W)))
            modg = mod.clone().requires_grad_(True)
            w, b = module.norm.weight, module.norm.bias
            es, ms = x.element_size(), mod.element_size()
            n = x.numel()
            fwd_bytes = n * es + 2 * n * ms + n * 4
            bwd_bytes = n * es + n * ms + n * 4 + n * es + 2 * n * ms            # x + scale half + g, d x + d mod

            def k_fwd():
                with torch.no_grad():
                    return motion.modln(x, mod, w, b, 1e-6)

            def k_fwd_bwd():
                return torch.autograd.grad(motion.modln(xg, modg, w, b, 1e-6), [xg, modg, w, b], gout)

            if args.trace:
                for fn in [make("native", c) for c in ("fwd", "fwd_bwd", "fwd_lift", "fwd_bwd_lift")]:
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                continue
            case = dict(B=B, dtype=str(dt).replace("torch.", ""), V=V, C=C, H=H, W=W)
            for name in ("fwd", "fwd_bwd", "fwd_lift", "fwd_bwd_lift"):
                fa, fb = make("native", name), make("reference", name)
                ra, rb = timed_pair(fa, fb, args.reps)
                for side, r, fn in (("native", ra, fa), ("reference", rb, fb)):
                    lines.append(dict(case, case=name, side=side, ms=round(r[0], 4), ms_min=round(r[1], 4), ms_max=round(r[2], 4), reps=args.reps,
                                      peak_mb=round(peak(fn), 1)))
                    print(json.dumps(lines[-1]), flush=True)
                verdicts.append(dict(case=name, B=B, dtype=case["dtype"], ok=bool(ra[0] < rb[0] and ra[2] < rb[1]), speedup=round(rb[0] / ra[0], 2)))
            rf, rfb = timed_pair(k_fwd, k_fwd_bwd, args.reps)
            lines.append(dict(case, case="modln_fwd", side="native", ms=round(rf[0], 4), ms_min=round(rf[1], 4), ms_max=round(rf[2], 4), reps=args.reps,
                              algo_mb=round(fwd_bytes / 1e6, 1), algo_tbs=round(fwd_bytes / rf[0] / 1e9, 3)))
            print(json.dumps(lines[-1]), flush=True)
            lines.append(dict(case, case="modln_fwd_bwd", side="native", ms=round(rfb[0], 4), ms_min=round(rfb[1], 4), ms_max=round(rfb[2], 4),
                              reps=args.reps, algo_mb=round((fwd_bytes + bwd_bytes) / 1e6, 1),
                              algo_tbs=round((fwd_bytes + bwd_bytes) / rfb[0] / 1e9, 3)))
            print(json.dumps(lines[-1]), flush=True)
            del x, xg, mod, modg
    if not args.trace:
        lines.append(dict(case="merge_condition", holds=all(v["ok"] for v in verdicts), cases=verdicts))
        print(json.dumps(lines[-1]), flush=True)
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
