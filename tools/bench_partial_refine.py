"""ms / step of the masked refine step (refine_item / mask, igs_refine_step_masked) on the cfg3 scene, one JSON line on stdout.

Cases, each with the L1 and the L1 + SSIM loss (200k Gaussians, 1352 x 1014, ten training cameras, Morton-sorted store):
  plain      the unmasked fused step (igs_refine_step)
  trivial    the same store through igs_refine_step_masked with {0, 0}
  dynamic    SyntheticStream's dynamic-bbox mask (use_mask)
  idx20      a random 20 % index mask
  idx50      a random 50 % index mask
  no_shs     refine_item.no_shs, no mask
  plain_end  the plain step again at the end (run-to-run spread of this process)
Timing: device-synchronised wall clock over --steps steps after --warmup steps, one store per case.  With --psnr every case also
runs one fresh 50-iteration frame and reports the held-out view's PSNR after it.

    python tools/bench_partial_refine.py [--steps 200] [--warmup 20] [--psnr]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--psnr", action="store_true", help="also the held-out PSNR after one 50-iteration frame per case")
    ap.add_argument("--frame-iters", type=int, default=50)
    ap.add_argument("--spinup-ms", type=float, default=300.0)
    ap.add_argument("--losses", default="l1,l1_ssim")
    ap.add_argument("--cases", default="plain,trivial,dynamic,idx20,idx50,no_shs,plain_end")
    args = ap.parse_args()
    if args.steps < 200:
        ap.error("--steps must be at least 200")

    import ctypes as C
    import torch
    from igs_amd import _cabi, rasterizer
    from igs_amd.refine import GaussianParams, Refiner, render, psnr
    from igs_amd.scenes import sear_steak_like_scene, perturbed_copy, activate
    from igs_amd.stream import SyntheticStream

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rasterizer.NAN_CHECKS = False
    raw, cams_all, bg = sear_steak_like_scene(P=args.points, held_out=True)
    cams_all = [c.to(dev) for c in cams_all]
    cams, test_cam = cams_all[:-1], cams_all[-1]
    bg = bg.to(dev)
    gt_raw = {k: v.to(dev) for k, v in perturbed_copy(raw).items()}
    with torch.no_grad():
        gts = [render(activate(gt_raw), c, bg)["images_pred"].clone() for c in cams]
        gt_test = render(activate(gt_raw), test_cam, bg)["images_pred"].clone()
    P = raw["xyz"].shape[0]
    gen = torch.Generator().manual_seed(2024)
    dynamic = SyntheticStream(raw, cams, bg, dev, start_sigma=0.0).dynamic.cpu()
    cases = dict(plain=dict(), trivial=dict(trivial=True), dynamic=dict(mask=dynamic),
                 idx20=dict(mask=torch.randperm(P, generator=gen)[: P // 5]),
                 idx50=dict(mask=torch.randperm(P, generator=gen)[: P // 2]),
                 no_shs=dict(refine_item=dict(no_shs=True)), plain_end=dict())
    L = _cabi.lib()
    plain_entry = L.igs_refine_step

    def make(spec, loss, seed=0):
        p = GaussianParams(raw, dev, refine_item=spec.get("refine_item"), mask=spec.get("mask"))
        p.spatial_sort()
        return p, Refiner(p, cams, gts, bg, loss=loss, seed=seed)

    def entry(spec):
        if spec.get("trivial"):
            m = _cabi.RefineMaskArgs(0, 0)
            masked = L.igs_refine_step_masked
            L.igs_refine_step = lambda a: masked(a, C.byref(m))
        else:
            L.igs_refine_step = plain_entry

    # device spin-up (untimed): the clocks ramp during the first tens of milliseconds of work
    _, r = make({}, "l1", seed=99)
    t = time.perf_counter()
    while (time.perf_counter() - t) * 1e3 < args.spinup_ms:
        for _ in range(20):
            r.step()
        torch.cuda.synchronize()
    del r

    results = {}
    for loss in args.losses.split(","):
        res = results[loss] = {}
        for name in args.cases.split(","):
            spec = cases[name]
            p, r = make(spec, loss)
            entry(spec)
            for _ in range(args.warmup):
                r.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                r.step()
            torch.cuda.synchronize()
            ms = 1000.0 * (time.perf_counter() - t0) / args.steps
            entry({})
            rec = dict(ms_per_step=round(ms, 4), trainable_from=p.trainable_from, mask_num=p.mask_num, frozen_groups=list(p.frozen_groups))
            del p, r
            if args.psnr:
                p, r = make(spec, loss, seed=1)
                entry(spec)
                for _ in range(args.frame_iters):
                    r.step()
                entry({})
                with torch.no_grad():
                    rec["psnr_after_frame"] = round(float(psnr(render(p.activated(), test_cam, bg)["images_pred"], gt_test)), 3)
                del p, r
            res[name] = rec
            print("[bench_partial_refine] %s %-9s %s" % (loss, name, rec), file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    with torch.no_grad():
        p0 = GaussianParams(raw, dev)
        psnr_start = float(psnr(render(p0.activated(), test_cam, bg)["images_pred"], gt_test))
    print(json.dumps(dict(metric="partial_refine_ms_per_step", unit="ms", points=P, width=1352, height=1014, views=len(cams),
                          steps=args.steps, warmup=args.warmup, frame_iters=args.frame_iters if args.psnr else None,
                          psnr_held_out_start=round(psnr_start, 3), results=results)))


if __name__ == "__main__":
    main()
