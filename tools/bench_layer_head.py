"""Timing of the fused q / k / v projections (proj.hip through igs_amd.tokens.project_tokens) against the nn.Linear calls they replace, on the
GPU, under no_grad.  JSON lines:

{"case": "launch" | "transformer", "side", "shape", "dtype", "n", "ms": median of HIP-event-timed calls, "ms_min", "ms_max", "reps",
 "peak_mb": peak memory above the operands}

  launch        one project_tokens call with n outputs on [32768, 128] and [163840, 128] rows against n F.linear calls on the same rows:
                 n = 5   the five products of a FeatureTransformer block's input, rot = (0, 0, 0, T / 2, T / 2), against the swap
                         torch.cat(x.chunk(2)[::-1]) and five F.linear (three of x, two of the swapped copy)
                 n = 3, 2, 1   against three, two, one F.linear
  transformer   a six-block stand-in FeatureTransformer (tests/layer_head_restatement.py) on two [4, 128, 64, 64] maps (8 x 4096 tokens),
                native window attention on every side:
                 heads          use_native_feature_transformer, every launch fused
                 heads, q eager the same with LAYER_HEAD_MIN_OUTPUTS = 2 (the cross layer's q stays nn.Linear)
                 tails          use_native_window_attention + use_native_layer_tails alone

  train         (--train only, written to its own file) forward + backward of one project_tokens_autograd call with n outputs (proj.hip and
                proj_bwd.hip) against n F.linear calls under autograd, plus the swap cat for n = 5, on the same rows and the same upstream
                gradients, one per output; x and every weight require a gradient; n = 1, 2, 3, 5 at both shapes

The sides of a case alternate inside one process; the operands rotate through more than twice the Infinity Cache.  float16 is autocast to
half on float32 rows, as the shipped models run.  The last line is {"case": "summary", "ratios": [...]}: for every case the other side's
median over the native one's and whether the two min - max ranges are disjoint.

usage: python tools/bench_layer_head.py [--reps 20] [--case launch|transformer|all] [--out FILE]
       python tools/bench_layer_head.py --train [--reps 20] [--out profiles/layer_head_train_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_attention import peak, timed_group  # noqa: E402
from bench_encoder_norms import Ring  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--case", default="all", choices=("launch", "transformer", "all"))
    ap.add_argument("--train", action="store_true", help="time forward + backward instead (the case 'train' alone)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.train:
        args.case = "train"
        args.out = args.out or os.path.join(ROOT, "profiles", "layer_head_train_bench.jsonl")
    assert torch.cuda.is_available(), "bench_layer_head needs a GPU"
    import layer_head_restatement as LH
    import token_ops_restatement as TR
    from igs_amd import attention as AT, tokens as TK
    dev = torch.device("cuda:0")
    lines, verdicts = [], []

    def record(case, sides, fns):
        res = timed_group(fns, args.reps)
        for side, r, fn in zip(sides, res, fns):
            ln = dict(case, side=side, ms=round(r[0], 4), ms_min=round(r[1], 4), ms_max=round(r[2], 4), reps=args.reps, peak_mb=round(peak(fn), 1))
            lines.append(ln)
            print(json.dumps(ln), flush=True)
        for side, r in list(zip(sides, res))[1:]:
            verdicts.append(dict(case, native=sides[0], against=side, speedup=round(r[0] / res[0][0], 2),
                                 disjoint=bool(res[0][2] < r[1] or r[2] < res[0][1])))

    if args.case in ("launch", "all"):
        for T in (32768, 163840):
            ring = Ring(lambda i: torch.randn(T, 128, device=dev), T * 128 * 4)
            for half in (False, True):
                cdt = torch.float16 if half else torch.float32
                for n in (5, 3, 2, 1):
                    ws = [torch.nn.Parameter(w) for w in LH.make_weights(n, n, torch.float32, dev)]
                    pack = TK.pack_projections(ws, cdt)
                    rot = (0, 0, 0, T // 2, T // 2) if n == 5 else None
                    case = dict(case="launch", shape=[T, 128], dtype="float16 (autocast)" if half else "float32", n=n)

                    def native():
                        return TK.project_tokens(ring.next(), ws, rot=rot, packed=pack, compute_dtype=cdt)

                    def eager():
                        x = ring.next()
                        if n == 5:
                            swapped = torch.cat(x.chunk(2, 0)[::-1], 0)
                            return [F.linear(x, w) for w in ws[:3]] + [F.linear(swapped, w) for w in ws[3:]]
                        return [F.linear(x, w) for w in ws]

                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
                        record(case, ("native", "eager"), [native, eager])
            del ring
            torch.cuda.empty_cache()

    if args.case == "train":
        for T in (32768, 163840):
            xs = Ring(lambda i: torch.randn(T, 128, device=dev).requires_grad_(True), T * 128 * 4)
            for half in (False, True):
                cdt = torch.float16 if half else torch.float32
                gs = Ring(lambda i: [torch.randn(T, 128, device=dev, dtype=cdt) for _ in range(5)], 5 * T * 128 * (2 if half else 4))
                for n in (5, 3, 2, 1):
                    ws = [torch.nn.Parameter(w) for w in LH.make_weights(n, n, torch.float32, dev)]
                    pack, pack_t = TK.pack_projections(ws, cdt, transposed=True)
                    rot = (0, 0, 0, T // 2, T // 2) if n == 5 else None
                    case = dict(case="train", shape=[T, 128], dtype="float16 (autocast)" if half else "float32", n=n)

                    def step(forward):
                        x, g = xs.next(), gs.next()[:n]
                        with torch.autocast("cuda", dtype=torch.float16, enabled=half):
                            outs = forward(x)
                        torch.autograd.backward(list(outs), g)
                        x.grad = None
                        for w in ws:
                            w.grad = None

                    def native_forward(x):
                        return TK.project_tokens_autograd(x, ws, rot=rot, packed=pack, packed_t=pack_t, compute_dtype=cdt)

                    def eager_forward(x):
                        if n == 5:
                            swapped = torch.cat(x.chunk(2, 0)[::-1], 0)
                            return [F.linear(x, w) for w in ws[:3]] + [F.linear(swapped, w) for w in ws[3:]]
                        return [F.linear(x, w) for w in ws]

                    record(case, ("native", "eager"), [lambda: step(native_forward), lambda: step(eager_forward)])
                del gs
                torch.cuda.empty_cache()
            del xs
            torch.cuda.empty_cache()

    if args.case in ("transformer", "all"):
        assert AT.use_native_window_attention(TR) == 2
        models = [LH.make_transformer(True, blocks=6).to(dev) for _ in range(3)]
        for m in models[1:]:
            m.load_state_dict(models[0].state_dict())
        assert TK.use_native_feature_transformer(models[0], True) == 12 and TK.use_native_feature_transformer(models[1], True) == 12
        assert TK.use_native_layer_tails(models[2]) == 12
        TK.LAYER_HEAD_FUSED = {torch.float32: True, torch.float16: True}
        ring = Ring(lambda i: (torch.randn(4, 128, 64, 64, device=dev), torch.randn(4, 128, 64, 64, device=dev)), 2 * 4 * 4096 * 128 * 4)

        def run(model, least):
            TK.LAYER_HEAD_MIN_OUTPUTS = {torch.float32: least, torch.float16: least}
            return model(*ring.next(), attn_type="swin", attn_num_splits=2)

        for half in (False, True):
            case = dict(case="transformer", shape=[8, 4096, 128], dtype="float16 (autocast)" if half else "float32", n=None)
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
                record(case, ("heads", "heads, q eager", "tails"), [lambda: run(models[0], 1), lambda: run(models[1], 2), lambda: run(models[2], 1)])

    lines.append(dict(case="summary", ratios=verdicts))
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
