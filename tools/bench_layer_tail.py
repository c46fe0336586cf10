"""Timing of the fused layer tail (ffn.hip through igs_amd.tokens.layer_tail) against the two ways the same work runs without it, on the
same GPU in the same process, the sides alternating.  One JSON line per case and side:
{"case": "tail" | "transformer", "side", "shape", "dtype", "has_ffn", "ms": median of HIP-event-timed calls, "ms_min", "ms_max", "reps",
 "peak_mb"}

  tail         everything behind the attention of one unimatch TransformerLayer (hidden 1024) at [32768, 128] (streaming, B = 1) and
               [16384, 128] (FeatureTransformerMy), with and without FFN, under torch.no_grad():
                 fused    layer_tail: one launch
                 unfused  the tail of the forward that use_native_transformer_layers binds: merge, layer_norm, cat, the two Linears around
                          the GELU, layer_norm with the residual
                 eager    unpatched PyTorch, the reference's `is_self_attn` test (sub, abs, max, compare) included
  transformer  a six-block stand-in FeatureTransformer (per block a layer without FFN on (source, source) and one with FFN on
               (source, target), the two images concatenated on the batch, 2 x 2 windows shifted by half a window in every second
               block, with the shift mask) at [8, 4096, 128], with the native window attention and use_native_transformer_layers on
               one side, use_native_layer_tails on top on the other
float32, and float16 under autocast (the attention's output is half there, source float32, as in the bound forward).  Every call takes the
next of a ring of operand sets larger than twice the 256 MiB Infinity Cache; the weights are one fixed set, as in use.  The last line
lists the ratios against the fused side and whether the min-max ranges are disjoint.

The tool sets no time limit of its own.  --case is the unit to run under one: each case is one process that ends after its last line,
    timeout -k 10 400 python tools/bench_layer_tail.py --case tail --out tail.jsonl \
      && timeout -k 10 300 python tools/bench_layer_tail.py --case transformer --out transformer.jsonl
and profiles/layer_tail_bench.jsonl is the two files one after the other.

--train times a training step instead (profiles/layer_tail_train_bench.jsonl): the forward plus backward() of the same modules with every
.grad reset before the step, the inputs and the parameters of the tail requiring grad.
                 native   layer_tail_autograd (tail) / use_native_layer_tails(training=True) with LAYER_TAIL_BWD_NATIVE forced on and the
                          fill rule off (transformer): the fused forward, the recomputing backward of ffn_bwd.hip
                 unfused  today's training path: use_native_transformer_layers' tail under autograd
The native tail steps run on packs made once; what a step after an optimiser update adds is timed on its own as side "repack" (both
packs of pack_layer_tail(..., transposed=True)).  peak_mb is the step's peak above the operands, the forward's saved tensors included.

usage: python tools/bench_layer_tail.py [--reps 20] [--case tail|transformer|all] [--train] [--out FILE]
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
import torch.nn as nn  # noqa: E402

from bench_attention import peak, timed_group  # noqa: E402
from bench_encoder_norms import Ring  # noqa: E402


class Block(nn.Module):
    """unimatch's TransformerBlock: self-attention without FFN, then cross-attention with the FFN."""

    def __init__(self, seed):
        super().__init__()
        import token_ops_restatement as TR
        self.self_attn = TR.make_layer(128, no_ffn=True, seed=seed)
        self.cross_attn_ffn = TR.make_layer(128, no_ffn=False, seed=seed + 100)

    def forward(self, source, target, **kw):
        return self.cross_attn_ffn(self.self_attn(source, source, **kw), target, **kw)


class StandInTransformer(nn.Module):
    """The layer loop of unimatch's FeatureTransformer: both images on the batch, the second half swapped in as the target."""

    def __init__(self, blocks=6):
        super().__init__()
        self.layers = nn.ModuleList([Block(i) for i in range(blocks)])

    def forward(self, f0, f1, **kw):
        c0, c1 = torch.cat([f0, f1], 0), torch.cat([f1, f0], 0)
        for i, layer in enumerate(self.layers):
            c0 = layer(c0, c1, with_shift=i % 2 == 1, **kw)
            c1 = torch.cat(c0.chunk(2, 0)[::-1], 0)
        return c0.chunk(2, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--case", default="all", choices=("tail", "transformer", "all"))
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_layer_tail needs a GPU"
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
            verdicts.append(dict(case, fused_against=side, speedup=round(r[0] / res[0][0], 2), disjoint=bool(res[0][2] < r[1] or r[2] < res[0][1])))

    def eager_tail(layer, a, s, t):
        same = (s - t).abs().max() < 1e-6                              # noqa: F841  (the reference's dead test)
        m = layer.norm1(layer.merge(a))
        if not layer.no_ffn:
            m = layer.norm2(layer.mlp(torch.cat([s, m], dim=-1)))
        return s + m

    def step(module_params, fn, inputs):
        """One training step: .grad reset, forward, backward() of the sum against a fixed upstream gradient."""
        for p in module_params:
            p.grad = None
        leaves = [t.detach().requires_grad_(True) for t in inputs]
        out = fn(*leaves)
        out = out if torch.is_tensor(out) else torch.cat(list(out), 0)
        out.backward(torch.ones_like(out))
        return None

    if args.train and args.case in ("tail", "all"):
        for half in (False, True):
            adt = torch.float16 if half else torch.float32
            cdt = adt
            for T in (32768, 16384):
                ring = Ring(lambda i: (torch.randn(T, 128, device=dev).to(adt), torch.randn(T, 128, device=dev)), T * 128 * (4 + (2 if half else 4)))
                for no_ffn in (False, True):
                    layer = TR.make_layer(128, no_ffn=no_ffn, seed=1).to(dev)
                    params = TK._tail_params(layer)
                    pack, pack_t = TK.pack_layer_tail(layer, cdt, transposed=True)
                    case = dict(case="tail", mode="train", shape=[T, 128], dtype="float16 (autocast)" if half else "float32", has_ffn=not no_ffn)
                    native = lambda: step(params, lambda a, s: TK.layer_tail_autograd(a, s, layer, packed=pack, packed_t=pack_t, compute_dtype=cdt), ring.next())
                    unfused = lambda: step(params, lambda a, s: TK._layer_tail_unfused(layer, a, s), ring.next())
                    repack = lambda: TK.pack_layer_tail(layer, cdt, transposed=True)
                    with torch.autocast("cuda", dtype=torch.float16, enabled=half):
                        record(case, ("native", "unfused", "repack"), [native, unfused, repack])
                    verdicts.pop()                                     # (the repack is a part of a step, not a rival)
                del ring
                torch.cuda.empty_cache()

    if args.train and args.case in ("transformer", "all"):
        assert AT.use_native_window_attention(TR) == 2
        TK.LAYER_TAIL_BWD_NATIVE = {torch.float32: True, torch.float16: True}
        TK.LAYER_TAIL_FFN_MIN_FILL = {torch.float32: 0.0, torch.float16: 0.0}
        models = [StandInTransformer().to(dev) for _ in range(2)]
        models[1].load_state_dict(models[0].state_dict())
        assert TK.use_native_layer_tails(models[0], training=True) == 12 and TK.use_native_transformer_layers(models[1]) == 12
        ring = Ring(lambda i: (torch.randn(4, 4096, 128, device=dev), torch.randn(4, 4096, 128, device=dev)), 2 * 4 * 4096 * 128 * 4)
        import window_attention_restatement as WR
        kw = dict(height=64, width=64, attn_num_splits=2, shifted_window_attn_mask=WR.paint_mask(64, 64, 2).float().to(dev))
        for half in (False, True):
            case = dict(case="transformer", mode="train", shape=[8, 4096, 128], dtype="float16 (autocast)" if half else "float32", has_ffn=True)
            fns = [lambda m=m: step(list(m.parameters()), lambda f0, f1: m(f0, f1, **kw), ring.next()) for m in models]
            with torch.autocast("cuda", dtype=torch.float16, enabled=half):
                record(case, ("native", "unfused"), fns)

    if not args.train and args.case in ("tail", "all"):
        for half in (False, True):
            adt = torch.float16 if half else torch.float32
            for T in (32768, 16384):
                ring = Ring(lambda i: (torch.randn(T, 128, device=dev).to(adt), torch.randn(T, 128, device=dev), torch.randn(T, 128, device=dev)),
                            T * 128 * (8 + (2 if half else 4)))
                for no_ffn in (False, True):
                    layer = TR.make_layer(128, no_ffn=no_ffn, seed=1).to(dev)
                    cdt = torch.float16 if half else torch.float32
                    pack = TK.pack_layer_tail(layer, cdt)
                    case = dict(case="tail", shape=[T, 128], dtype="float16 (autocast)" if half else "float32", has_ffn=not no_ffn)

                    def fused():
                        a, s, _ = ring.next()
                        return TK.layer_tail(a, s, layer, packed=pack, compute_dtype=cdt)

                    def unfused():
                        a, s, _ = ring.next()
                        return TK._layer_tail_unfused(layer, a, s)

                    def eager():
                        return eager_tail(layer, *ring.next())

                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
                        record(case, ("fused", "unfused", "eager"), [fused, unfused, eager])
                del ring
                torch.cuda.empty_cache()

    if not args.train and args.case in ("transformer", "all"):
        assert AT.use_native_window_attention(TR) == 2
        models = [StandInTransformer().to(dev) for _ in range(2)]
        models[1].load_state_dict(models[0].state_dict())
        assert TK.use_native_layer_tails(models[0]) == 12 and TK.use_native_transformer_layers(models[1]) == 12
        ring = Ring(lambda i: (torch.randn(4, 4096, 128, device=dev), torch.randn(4, 4096, 128, device=dev)), 2 * 4 * 4096 * 128 * 4)
        import window_attention_restatement as WR
        kw = dict(height=64, width=64, attn_num_splits=2, shifted_window_attn_mask=WR.paint_mask(64, 64, 2).float().to(dev))
        for half in (False, True):
            case = dict(case="transformer", shape=[8, 4096, 128], dtype="float16 (autocast)" if half else "float32", has_ffn=True)
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
                record(case, ("with layer tails", "without"), [lambda: models[0](*ring.next(), **kw), lambda: models[1](*ring.next(), **kw)])

    lines.append(dict(case="summary", ratios=verdicts))
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
