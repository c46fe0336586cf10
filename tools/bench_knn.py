"""Timing of simple_knn.distCUDA2 (knn.hip: igs_knn_mean_dist2).  Prints one JSON line per case:
  {"case": "knn", "cloud": "uniform" | "clustered", "n": N, "ms": median over HIP-event-timed calls, "ms_min", "ms_max", "reps"}
and, with --brute, one line for a chunked float32 torch brute force at 100k points (for scale).

  uniform    N points uniform in the unit cube
  clustered  12 Gaussian blobs of widths 0.01..0.31 (centres ~N(0, 3)) plus 1 % outliers at 1000..2000 (a COLMAP cloud with sky)

usage: python tools/bench_knn.py [--sizes 100000,1000000,4000000] [--reps 20] [--brute] [--trace]
  --trace: 3 calls per case and no timing lines (for a rocprofv3 --kernel-trace --stats run)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def uniform(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, generator=g)


def clustered(n, seed=0, outliers=0.01, blobs=12, far=1000.0):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(blobs, 3, generator=g) * 3.0
    widths = torch.rand(blobs, generator=g) * 0.3 + 0.01
    k = torch.randint(0, blobs, (n,), generator=g)
    x = centres[k] + torch.randn(n, 3, generator=g) * widths[k, None]
    m = int(n * outliers)
    d = torch.nn.functional.normalize(torch.randn(m, 3, generator=g), dim=1)
    x[torch.randperm(n, generator=g)[:m]] = d * (far * (1 + torch.rand(m, 1, generator=g)))
    return x.float()


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


def brute_f32(x, chunk=256):
    out = torch.empty(x.shape[0], device=x.device)
    for a in range(0, x.shape[0], chunk):
        q = x[a:a + chunk]
        d = ((q[:, None, :] - x[None, :, :]) ** 2).sum(-1)
        d[torch.arange(q.shape[0], device=x.device), torch.arange(a, a + q.shape[0], device=x.device)] = float("inf")
        out[a:a + chunk] = torch.topk(d, 3, dim=1, largest=False).values.mean(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,4000000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--brute", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_knn needs a GPU"
    from simple_knn._C import distCUDA2
    dev = torch.device("cuda:0")
    for n in [int(s) for s in args.sizes.split(",")]:
        for name, make in (("uniform", uniform), ("clustered", clustered)):
            x = make(n, seed=n).to(dev)
            if args.trace:
                for _ in range(3):
                    distCUDA2(x)
                torch.cuda.synchronize()
                continue
            med, lo, hi = timed(lambda: distCUDA2(x), args.reps)
            print(json.dumps(dict(case="knn", cloud=name, n=n, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), reps=args.reps)),
                  flush=True)
    if args.brute and not args.trace:
        x = uniform(100000, seed=1).to(dev)
        med, lo, hi = timed(lambda: brute_f32(x), 3, warmup=1)
        print(json.dumps(dict(case="torch_brute_f32", cloud="uniform", n=100000, ms=round(med, 2), ms_min=round(lo, 2), ms_max=round(hi, 2),
                              reps=3)), flush=True)


if __name__ == "__main__":
    main()
