"""Timing of the anchor graph (anchors.hip through igs_amd.anchors and the torch_cluster / fpsample drop-ins).  Prints one JSON line per
case: {"case", "n", ..., "ms": median over HIP-event-timed calls, "ms_min", "ms_max", "reps"}.

  knn           k = 8 neighbours of N uniform points among 8192 uniform anchors (200k and 1M points)
  fps           N -> 8192 samples: uniform 200k, the sear_steak-like scene's 200k xyz, uniform 1M
  anchor_graph  get_mask_fpsample natively: B examples of the sear_steak-like scene, each with its own box (B = 1 and B = 5)
  dropin        the reference's own path: fpsample on a numpy array (host round trip included) + torch_cluster.knn

usage: python tools/bench_anchors.py [--reps 20] [--only knn,fps,anchor_graph,dropin] [--trace]
  --trace: 3 calls per case and no timing lines (for a rocprofv3 --kernel-trace --stats run)
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
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


def emit(args, fn, **case):
    if args.trace:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        return
    med, lo, hi = timed(fn, args.reps)
    print(json.dumps(dict(case, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), reps=args.reps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="knn,fps,anchor_graph,dropin")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_anchors needs a GPU"
    from igs_amd import anchors as A
    from igs_amd import scenes
    dev = torch.device("cuda:0")
    only = set(args.only.split(","))
    i32 = dict(dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(0)
    steak = scenes.sear_steak_like_scene(P=1000000)[0]["xyz"].float()

    if "knn" in only:
        anchors = torch.rand(8192, 3, generator=g).to(dev)
        for n in (200000, 1000000):
            pts = torch.rand(n, 3, generator=g).to(dev)
            px, py = torch.tensor([0, 8192], **i32), torch.tensor([0, n], **i32)
            emit(args, lambda: A.knn_native(anchors, pts, 8, px, py), case="knn", n=n, anchors=8192, k=8)
            emit(args, lambda: A.knn_native(anchors, pts, 8, px, py, weight_scale=10.0), case="knn_weights", n=n, anchors=8192, k=8)

    if "fps" in only:
        clouds = (("uniform", torch.rand(200000, 3, generator=g)), ("sear_steak", steak[:200000]),
                  ("uniform", torch.rand(1000000, 3, generator=g)))
        for name, x in clouds:
            x = x.to(dev)
            n = x.shape[0]
            emit(args, lambda: A.fps_native(x, torch.tensor([0, n], **i32), torch.tensor([0], **i32), torch.tensor([0, 8192], **i32), 8192, n,
                                            math.inf), case="fps", cloud=name, n=n, samples=8192)

    if "anchor_graph" in only:
        from igs_amd.scenes import SEAR_STEAK_BBOX
        bb = torch.tensor(SEAR_STEAK_BBOX)
        for B in (1, 5):
            xyz = [steak[b * 200000:(b + 1) * 200000].to(dev) for b in range(B)]
            box = torch.stack([bb + 0.1 * b for b in range(B)]).to(dev)
            emit(args, lambda: A.anchor_graph(xyz, box, 8192, 8, start_idx=[0] * B), case="anchor_graph", B=B, n_per_example=200000,
                 in_box=100000, anchors=8192, k=8)

    if "dropin" in only:
        import fpsample
        from torch_cluster import knn
        pc = steak[:200000].numpy()

        def dropin():
            s = fpsample.bucket_fps_kdline_sampling(pc, 8192, h=5, start_idx=0)
            pts = torch.from_numpy(pc).to(dev)
            anchors = pts[torch.from_numpy(s)]
            knn(anchors, pts, 8, torch.zeros(8192, device=dev, dtype=torch.long), torch.zeros(pts.shape[0], device=dev))
        emit(args, dropin, case="dropin_fpsample_knn", n=200000, anchors=8192, k=8)


if __name__ == "__main__":
    main()
