"""Timing of the multi-view anchor feature lift (lift.hip through igs_amd.motion.lift_anchor_features) against the reference's PyTorch
lines on the same GPU in the same process, alternating.  One JSON line per case:
{"case", "B", "dtype", "layout", "ms": median of HIP-event-timed calls, "ms_min", "ms_max", "reps", "peak_mb", "algo_mb", "algo_tbs"}.

  lift_fwd / lift_fwd_ref   forward under no_grad: native vs grid_encoder.py:84-88 + ops.py:444-477 (inverse, two matmuls, divide,
                            normalise, F.grid_sample, permute, mean)
  lift_bwd / lift_bwd_ref   forward + backward to the features
Shipped shape: V = 4, C = 128, 128 x 128 maps, A = 8192 anchors per example; B = 1 and 5; float32 and float16; NCHW and channels-last
(channels-last goes through a copy to NCHW on the native side: there are no channels-last kernels).  The reference always gets what it
gets in IGS: `motion_feature.to(torch.float)`.
algo_mb: the algorithmic bytes of the forward (features once + 12-byte sample table + float32 output; the backward: d out + table +
d feat), algo_tbs = algo bytes / median time.  peak_mb: growth of torch.cuda.max_memory_allocated() over the call.

usage: python tools/bench_lift.py [--reps 20] [--trace] [--out profiles/lift_bench.jsonl]
  --trace: 3 calls per native case and no timing (for a rocprofv3 --kernel-trace --stats run)
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
import torch.nn.functional as F  # noqa: E402


def ref_lift(feat, pts, c2w, K, B):
    """The reference's composition, in its own operations."""
    V = feat.shape[0] // B
    p = pts.unsqueeze(1).repeat_interleave(V, 1).reshape(B * V, -1, 3)
    w2c = torch.inverse(c2w)
    cam = torch.matmul(w2c[:, :3, :3], p.permute(0, 2, 1)) + w2c[:, :3, 3].unsqueeze(2)
    img = torch.matmul(K, cam)
    img = img / img[:, 2, :].unsqueeze(1)
    img = img[:, :2, :]
    _, _, H, W = feat.shape
    n = img.clone()
    n[:, 0, :] = 2 * n[:, 0, :] / W - 1
    n[:, 1, :] = 2 * n[:, 1, :] / H - 1
    grid = n.unsqueeze(1).permute(0, 1, 3, 2)
    s = F.grid_sample(feat.to(torch.float), grid, align_corners=False)
    s = s.squeeze(2).permute(0, 2, 1)
    return s.reshape(B, V, -1, s.shape[-1]).mean(dim=1)


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
    assert torch.cuda.is_available(), "bench_lift needs a GPU"
    from igs_amd import motion
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    V, C, H, W, A = 4, 128, 128, 128, 8192
    lines = []
    for B in (1, 5):
        c2w = torch.eye(4).repeat(B * V, 1, 1)
        c2w[:, :3, :3] += 0.1 * torch.randn(B * V, 3, 3, generator=g)
        c2w[:, :3, 3] = torch.tensor([0.0, 0.0, -3.0]) + 0.3 * torch.randn(B * V, 3, generator=g)
        c2w = c2w.to(dev)
        pts = (torch.rand(B, A, 3, generator=g) * 3.0 - 1.5).to(dev)
        K = torch.eye(3).repeat(B * V, 1, 1)
        K[:, 0, 0] = K[:, 1, 1] = 140.0
        K[:, 0, 2] = K[:, 1, 2] = 64.0
        K = K.to(dev)
        intr = torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1).contiguous()
        gout = torch.randn(B, A, C, generator=g).to(dev)
        for dt in (torch.float32, torch.float16):
            for layout in ("nchw", "channels_last"):
                feat = torch.randn(B * V, C, H, W, generator=g).to(dt).to(dev)
                if layout == "channels_last":
                    feat = feat.contiguous(memory_format=torch.channels_last)
                es = feat.element_size()
                fwd_bytes = feat.numel() * es + B * V * A * 12 + B * A * C * 4
                bwd_bytes = B * A * C * 4 + B * V * A * 12 + feat.numel() * es
                fg = feat.clone().requires_grad_(True)

                def nat_f():
                    with torch.no_grad():
                        return motion.lift_anchor_features(feat, pts, c2w, intr)

                def ref_f():
                    with torch.no_grad():
                        return ref_lift(feat, pts, c2w, K, B)

                def nat_b():
                    return torch.autograd.grad(motion.lift_anchor_features(fg, pts, c2w, intr), fg, gout)

                def ref_b():
                    return torch.autograd.grad(ref_lift(fg, pts, c2w, K, B), fg, gout)

                if args.trace:
                    for fn in (nat_f, nat_b):
                        for _ in range(3):
                            fn()
                    torch.cuda.synchronize()
                    continue
                case = dict(B=B, dtype=str(dt).replace("torch.", ""), layout=layout, V=V, C=C, H=H, W=W, A=A)
                for (na, nb, fa, fb, by) in (("lift_fwd", "lift_fwd_ref", nat_f, ref_f, fwd_bytes),
                                             ("lift_bwd", "lift_bwd_ref", nat_b, ref_b, fwd_bytes + bwd_bytes)):
                    ra, rb = timed_pair(fa, fb, args.reps)
                    for name, r, fn in ((na, ra, fa), (nb, rb, fb)):
                        lines.append(dict(case, case=name, ms=round(r[0], 4), ms_min=round(r[1], 4), ms_max=round(r[2], 4), reps=args.reps,
                                          peak_mb=round(peak(fn), 1), algo_mb=round(by / 1e6, 2), algo_tbs=round(by / r[0] / 1e9, 3)))
                        print(json.dumps(lines[-1]), flush=True)
                del feat, fg
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
