"""Timing of one whole densify-and-prune event -- plan, igs_densify_remap, statistics reset, synchronised at both ends -- with the
native plan (densify.hip through igs_amd.densify.plan_native, DensifyConfig(native=True)) against the PyTorch plan
(igs_amd.densify.plan), alternated call by call inside one process after a warm-up of both.

Store: P = 200000 and P = 20000 Gaussians with 16 SH coefficients (59 floats each, three flat buffers), random Adam moments.
Statistics: grad_accum uniform, denom in {1, 2, 3}, threshold at the 94 % quantile of g: about 6 % of the Gaussians are candidates;
percent_dense * extent at the median of the largest scale, so about half of them clone and half split; min_opacity prunes about 2 %.
Cases per P: "unbounded" (max_num far away) and "bounded" (max_num = P + 2 % of P: the top-k branch keeps a third of the candidates).
Before every timed call the store and the statistics are put back from copies (not timed).

Prints, and appends to --out, one JSON line per (P, case, path): {"P", "case", "path", "wall_ms": median host clock around the event
with a device synchronise at both ends, "event_ms": median of a HIP-event pair around it, their min / max, "reps", "P_new",
"n_clone", "n_split", "n_pruned", "launches": device kernels and copies of one event counted by torch.profiler (null if the
profiler is not available), "host_waits": device-to-host waits of the path, from its code, "same_decision": both paths gave equal
counts and equal src / fresh / ovr on the timed inputs (these are not moved off the thresholds as the tests' are, so one float32
rounding of exp or sigmoid can put a Gaussian in another class; tests/test_gpu_densify_native.py holds the equality)}.

usage: python tools/bench_densify.py [--reps 20] [--p 200000,20000] [--out profiles/densify_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HOST_WAITS = dict(native=1, torch=5)      # counts.tolist() | int(selected.sum()), three nonzero, int((~keep).sum()) (topk itself does not wait)


def make_case(P, dev, seed=0):
    from igs_amd.refine import GROUPS
    g = torch.Generator().manual_seed(seed)
    raw = dict(xyz=torch.rand(P, 3, generator=g) * 6.0 - 3.0, rotation=torch.randn(P, 4, generator=g),
               shs=torch.randn(P, 16, 3, generator=g) * 0.3, opacity=torch.randn(P, 1, generator=g) * 2.0 - 1.2,
               scaling=(torch.randn(P, 3, generator=g) * 0.8 - 4.0).clamp(-7.0, -1.0))
    accum = torch.rand(P, generator=g) * 6e-4
    denom = torch.randint(1, 4, (P,), generator=g).float()
    gq = accum / denom
    thr = float(torch.quantile(gq, 0.94))
    split_limit = float(torch.exp(raw["scaling"]).max(dim=1).values.median())
    per = sum(k for _, k in GROUPS)
    moments = (torch.randn(per * P, generator=g), torch.rand(per * P, generator=g))
    return raw, accum.to(dev), denom.to(dev), thr, split_limit, [m.to(dev) for m in moments]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--p", default="200000,20000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_densify needs a GPU"
    from igs_amd import densify as dn
    from igs_amd.refine import GaussianParams
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for P in [int(s) for s in args.p.split(",")]:
        raw, accum, denom, thr, split_limit, (m0, v0) = make_case(P, dev)
        params = GaussianParams(raw, dev)
        flat0 = params.flat.detach().clone()
        for case, max_num in (("unbounded", 100 * P), ("bounded", P + P // 50)):
            cfgs = {path: dn.DensifyConfig(grad_threshold=thr, min_opacity=0.005, max_num=max_num, percent_dense=split_limit, extent=1.0,
                                           native=(path == "native")) for path in ("native", "torch")}
            gens = {path: torch.Generator(device=dev).manual_seed(7) for path in cfgs}

            def restore():
                params._bind(P, flat0.clone(), m0.clone(), v0.clone())
                st = dn.DensifyState(P, dev)
                st.grad_accum.copy_(accum)
                st.denom.copy_(denom)
                return st

            def event(path, st):
                return dn.densify_and_prune(params, st, cfgs[path], gens[path])

            # ---- same decision on the timed inputs
            pls = {}
            for path in cfgs:
                pl = event(path, restore())
                pls[path] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in pl.items()}
            a, b = pls["native"], pls["torch"]
            same = all(a[k] == b[k] for k in ("n_clone", "n_split", "n_pruned")) and all(torch.equal(a[k], b[k]) for k in ("src", "fresh", "ovr"))
            # ---- timing, alternated
            for _ in range(3):
                for path in cfgs:
                    event(path, restore())
            wall, evt = {p_: [] for p_ in cfgs}, {p_: [] for p_ in cfgs}
            for _ in range(args.reps):
                for path in cfgs:
                    st = restore()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    event(path, st)
                    e1.record()
                    torch.cuda.synchronize()
                    wall[path].append((time.perf_counter() - t0) * 1e3)
                    evt[path].append(e0.elapsed_time(e1))
            launches = {}
            for path in cfgs:
                launches[path] = None
                try:
                    from torch.profiler import ProfilerActivity, profile
                    st = restore()
                    torch.cuda.synchronize()
                    with profile(activities=[ProfilerActivity.CUDA]) as prof:
                        event(path, st)
                        torch.cuda.synchronize()
                    launches[path] = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
                except Exception as exc:  # noqa: BLE001
                    print("bench_densify: torch.profiler not usable here (%s): launches not counted" % exc, file=sys.stderr)
            med = lambda v: sorted(v)[len(v) // 2]
            for path in cfgs:
                emit(dict(P=P, case=case, path=path, wall_ms=round(med(wall[path]), 4), wall_ms_min=round(min(wall[path]), 4),
                          wall_ms_max=round(max(wall[path]), 4), event_ms=round(med(evt[path]), 4), event_ms_min=round(min(evt[path]), 4),
                          event_ms_max=round(max(evt[path]), 4), reps=args.reps, P_new=int(pls[path]["src"].numel()),
                          n_clone=pls[path]["n_clone"], n_split=pls[path]["n_split"], n_pruned=pls[path]["n_pruned"],
                          launches=launches[path], host_waits=HOST_WAITS[path], same_decision=same))
        del params
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
