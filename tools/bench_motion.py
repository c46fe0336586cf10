"""Timing of the two anchor-graph consumers (motion.hip through igs_amd.motion) against the reference's PyTorch lines.  Prints one JSON
line per case: {"case", "n", "B", ..., "ms": median over HIP-event-timed calls, "ms_min", "ms_max", "reps", "peak_mb"}.

  interp_fwd / interp_fwd_ref   out = sum_k w * F[col] under no_grad: native launch vs gs.py:816-820's gather, product and sum
  interp_bwd / interp_bwd_ref   forward + backward to F and w (native: index build included) vs autograd through the same lines
  deform_fwd / deform_fwd_ref   xyz[mask] += dxyz, rot[mask] = qmul(nrm, nrm) vs gs.py:347-375 + general_utils.py:177-200 (two keys)
  deform_bwd / deform_bwd_ref   forward + backward to every input
Cases: N = 100k and 1M Gaussians, B = 1 and 5 (IGS's repeated layout), A = 8192 anchors per example, K = 8, D = 128.
peak_mb: torch.cuda.max_memory_allocated() growth over the call, in MB.

usage: python tools/bench_motion.py [--reps 20] [--only interp,deform] [--trace]
  --trace: 3 calls per case and no timing lines (for a rocprofv3 --kernel-trace --stats run)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def emit(args, fn, **case):
    if args.trace:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        return
    med, lo, hi = timed(fn, args.reps)
    print(json.dumps(dict(case, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), reps=args.reps, peak_mb=round(peak(fn), 1))),
          flush=True)


def ref_interp(F, w, col, K):
    """gs.py:816-820 in the reference's own operations."""
    f = F.reshape(-1, F.shape[-1])[col].view(-1, K, F.shape[-1])
    return torch.sum(f * w, dim=1)


def ref_qmul(a, b):
    a, b = torch.nn.functional.normalize(a), torch.nn.functional.normalize(b)
    w1, x1, y1, z1 = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    w2, x2, y2, z2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2, w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2], -1)


def ref_deform(xyz, rot, mask, dx, dr):
    xo, ro = xyz.clone(), rot.clone()
    ro[mask] = ref_qmul(ro[mask], dr.clone())
    xo[mask] = dx.clone() + xo[mask]
    return xo, ro


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="interp,deform")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_motion needs a GPU"
    from igs_amd import motion
    dev = torch.device("cuda:0")
    only = set(args.only.split(","))
    g = torch.Generator().manual_seed(0)
    A, K, D = 8192, 8, 128

    if "interp" in only:
        for n in (100000, 1000000):
            for B in (1, 5):
                F = torch.randn(B, A, D, generator=g).to(dev)
                ex = torch.arange(n) * B // n
                col = (torch.randint(0, A, (n, K), generator=g) + ex[:, None] * A).reshape(-1).to(dev)
                w = torch.softmax(torch.randn(n, K, generator=g), 1).unsqueeze(-1).to(dev)
                dout = torch.randn(n, D, generator=g).to(dev)
                case = dict(n=n, B=B, anchors=A, k=K, d=D)
                with torch.no_grad():
                    emit(args, lambda: motion.interpolate_anchor_features(F, w, col), case="interp_fwd", **case)
                    emit(args, lambda: ref_interp(F, w, col, K), case="interp_fwd_ref", **case)
                Fg, wg = F.clone().requires_grad_(True), w.clone().requires_grad_(True)
                emit(args, lambda: torch.autograd.grad(motion.interpolate_anchor_features(Fg, wg, col), (Fg, wg), dout), case="interp_bwd", **case)
                emit(args, lambda: torch.autograd.grad(ref_interp(Fg, wg, col, K), (Fg, wg), dout), case="interp_bwd_ref", **case)
                del F, col, w, dout, Fg, wg

    if "deform" in only:
        for n in (100000, 1000000):
            P = 2 * n                                    # the masked (in-box) Gaussians are half of the set
            xyz = torch.randn(P, 3, generator=g).to(dev)
            rot = torch.randn(P, 4, generator=g).to(dev)
            mask = torch.randperm(P, generator=g)[:n].sort().values.to(dev)
            dx = (torch.randn(n, 3, generator=g) * 0.01).to(dev)
            dr = torch.randn(n, 4, generator=g).to(dev)
            gx, gr = torch.randn(P, 3, generator=g).to(dev), torch.randn(P, 4, generator=g).to(dev)
            case = dict(n=n, P=P)
            with torch.no_grad():
                emit(args, lambda: motion.deform_xyz_rotation(xyz, rot, mask, dx, dr), case="deform_fwd", **case)
                emit(args, lambda: ref_deform(xyz, rot, mask, dx, dr), case="deform_fwd_ref", **case)
            leaves = [t.clone().requires_grad_(True) for t in (xyz, rot, dx, dr)]
            emit(args, lambda: torch.autograd.grad(motion.deform_xyz_rotation(leaves[0], leaves[1], mask, leaves[2], leaves[3]), leaves, (gx, gr)),
                 case="deform_bwd", **case)
            emit(args, lambda: torch.autograd.grad(ref_deform(leaves[0], leaves[1], mask, leaves[2], leaves[3]), leaves, (gx, gr)),
                 case="deform_bwd_ref", **case)


if __name__ == "__main__":
    main()
