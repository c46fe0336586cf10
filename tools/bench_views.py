"""Forward + backward of V views of one Gaussian set: `rasterize_views` (one autograd node, one host wait, gradients summed by the
per-Gaussian kernel) against the per-view loop through `_RasterizeGaussians` with PyTorch accumulating the gradients -- the view loop
of igs/models/gs.py:839-847 as the drop-in packages run it.

Scene: sear_steak_like_scene, 200k Gaussians at 1352 x 1014 (the shipped training shape), V = 1, 5, 8 of its cameras; upstream
gradients: random on the colour image ("colour") or on the colour and the expected-depth image ("colour+depth"), handed to
torch.autograd.backward directly so that no loss kernels are timed on either side.  Both sides use the clamp variant's Function
(gs.py:591-611 uses the rade_clamp package) when --clamp is given, the plain one otherwise.

Per case the two sides are warmed up, then alternated call by call; every call is timed by the host clock between two device
synchronisations.  Prints, and appends to --out, one JSON line per (V, loss): {"V", "loss", "views_ms" / "loop_ms": median,
"views_min_ms", "views_max_ms", "loop_min_ms", "loop_max_ms", "reps", "views_peak_mb" / "loop_peak_mb":
torch.cuda.max_memory_allocated over one call, "views_launches" / "loop_launches": device kernels and copies of one call counted by
torch.profiler (null if unavailable), "max_rel_diff": largest difference between the two sides' gradients relative to the tensor's
largest entry (summation order differs: float32 rounding)}.

usage: python tools/bench_views.py [--reps 15] [--views 1,5,8] [--p 200000] [--out profiles/views_bench.jsonl] [--clamp]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def count_launches(fn):
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception:  # noqa: BLE001
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--views", default="1,5,8")
    ap.add_argument("--p", type=int, default=200000)
    ap.add_argument("--width", type=int, default=1352)
    ap.add_argument("--height", type=int, default=1014)
    ap.add_argument("--clamp", action="store_true")
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_views needs a GPU"
    from igs_amd import rasterizer as R
    from igs_amd.scenes import sear_steak_like_scene, activate
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, "a")
    E = torch.Tensor([])
    raw, cams, bg = sear_steak_like_scene(P=args.p, n_cams=10, width=args.width, height=args.height)
    bg = bg.to(dev)
    leaves = {k: v.to(dev).requires_grad_(True) for k, v in activate(raw).items()}
    names = ("means3D", "shs", "opacities", "scales", "rotations")
    single = R._RasterizeGaussiansClamp if args.clamp else R._RasterizeGaussians
    H, W = cams[0].height, cams[0].width

    def settings(cam=None):
        return R.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=cams[0].tanfovx, tanfovy=cams[0].tanfovy, kernel_size=0.0, bg=bg, scale_modifier=1.0,
            viewmatrix=E if cam is None else cam.world_view_transform.to(dev), projmatrix=E if cam is None else cam.full_proj_transform.to(dev),
            sh_degree=3, campos=E if cam is None else cam.camera_center.to(dev), prefiltered=False, require_depth=True, require_coord=True,
            debug=False)

    for V in [int(s) for s in args.views.split(",")]:
        use = cams[:V]
        per_view = [settings(c) for c in use]
        shared = settings()
        Vm = torch.stack([c.world_view_transform for c in use]).to(dev)
        Pm = torch.stack([c.full_proj_transform for c in use]).to(dev)
        Cc = torch.stack([c.camera_center for c in use]).to(dev)
        gen = torch.Generator().manual_seed(V)
        GC = torch.randn(V, 3, H, W, generator=gen).to(dev)
        GD = torch.randn(V, 1, H, W, generator=gen).to(dev)
        for loss in ("colour", "colour+depth"):
            depth = loss != "colour"

            def zero():
                for t in leaves.values():
                    t.grad = None

            def run_views():
                o = R.rasterize_views(leaves["means3D"], leaves["shs"], E, leaves["opacities"], leaves["scales"], leaves["rotations"], E, shared,
                                      Vm, Pm, Cc, clamp=args.clamp)
                torch.autograd.backward([o[0], o[4]] if depth else [o[0]], [GC, GD] if depth else [GC])

            def run_loop():
                outs, gs = [], []
                for v in range(V):
                    m2d = torch.zeros_like(leaves["means3D"], requires_grad=True)      # (screenspace_points of gs.py:583)
                    o = single.apply(leaves["means3D"], m2d, leaves["shs"], E, leaves["opacities"], leaves["scales"], leaves["rotations"], E,
                                     per_view[v])
                    outs.append(o[0]); gs.append(GC[v])
                    if depth:
                        outs.append(o[4]); gs.append(GD[v])
                torch.autograd.backward(outs, gs)

            def timed(fn):
                zero()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            def peak(fn):
                zero()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                fn()
                torch.cuda.synchronize()
                return torch.cuda.max_memory_allocated() / 2.0 ** 20

            for _ in range(3):
                timed(run_views); timed(run_loop)
            zero(); run_views(); torch.cuda.synchronize()
            g_views = {n: leaves[n].grad.clone() for n in names}
            zero(); run_loop(); torch.cuda.synchronize()
            diff = max(float((leaves[n].grad - g_views[n]).abs().max() / leaves[n].grad.abs().max().clamp_min(1e-30)) for n in names)
            tv, tl = [], []
            for _ in range(args.reps):
                tv.append(timed(run_views)); tl.append(timed(run_loop))
            rec = dict(V=V, loss=loss, clamp=bool(args.clamp), P=args.p, width=W, height=H, reps=args.reps,
                       views_ms=statistics.median(tv), views_min_ms=min(tv), views_max_ms=max(tv),
                       loop_ms=statistics.median(tl), loop_min_ms=min(tl), loop_max_ms=max(tl),
                       views_peak_mb=peak(run_views), loop_peak_mb=peak(run_loop),
                       views_launches=None if args.no_launches else count_launches(run_views),
                       loop_launches=None if args.no_launches else count_launches(run_loop), max_rel_diff=diff)
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
