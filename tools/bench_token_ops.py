"""Timing of the native LayerNorm and GEGLU (tokens.hip through igs_amd.tokens) against the same steps in eager PyTorch, on the same GPU in
the same process, alternating.  One JSON line per case and side:
{"case": "layer_norm" | "layer_tail" | "geglu" | "block" | "layer", "side": "native" | "eager", "shape", "dtype", "mode": "fwd" | "fwd+bwd",
 "ms": median of HIP-event-timed calls, "ms_min", "ms_max", "reps", "peak_mb", "bytes_mb": the unavoidable bytes (one read of every operand,
 one write of every result), "of_roof": bytes / ms against the measured 6.29 TB/s copy roof}

  layer_norm  nn.LayerNorm(512) at [8192 B, 512], B = 1, 5: F.layer_norm against layer_norm
  layer_tail  the end of a unimatch TransformerLayer at [16 * 4096, 128] and [8 * 4096, 128]: the dead `is_self_attn` test (sub, abs, max),
              F.layer_norm and `source + message` against layer_norm(residual=source)
  geglu       [8192 B, 4096] -> [8192 B, 2048]: chunk, F.gelu, multiply against geglu
  block       one stand-in BasicTransformerBlock (dim 512, 8 heads through F.scaled_dot_product_attention) at [1, 8192, 512] float32,
              unpatched against use_native_block_ops
  layer       one stand-in TransformerLayer with its FFN at [4, 64 * 64, 128] float32, K = 2, the restated window attention on both sides,
              unpatched against use_native_transformer_layers
float32 and float16, forward and forward + backward (autograd.grad to the inputs and parameters).  Every call takes the next of a ring of
operand sets larger than twice the 256 MiB Infinity Cache, so that neither side reads its inputs from it; for the whole block and layer the
inputs rotate through such a ring and the weights are one fixed set per module, as in use.  In float16 the eager LayerNorm gets float16
parameters cast once outside the timed calls (F.layer_norm wants one dtype; a float16 module holds them so) and the native side the
float32 parameters as they are: neither side casts inside a timed call.  The last line lists, per case,
native against eager: speed-up and whether the min-max ranges are disjoint.

usage: python tools/bench_token_ops.py [--reps 20] [--out profiles/token_ops_bench.jsonl]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_attention import DefaultProcessor, peak, timed_group  # noqa: E402
from bench_encoder_norms import Ring  # noqa: E402

ROOF_TBS = 6.29
EPS = 1e-5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_token_ops needs a GPU"
    import attention_restatement as AR
    import token_ops_restatement as TR
    from igs_amd import tokens as TK
    dev = torch.device("cuda:0")
    lines, verdicts = [], []

    def record(case, fns, bytes_mb):
        res = timed_group(fns, args.reps)
        for side, r, fn in zip(("native", "eager"), res, fns):
            ln = dict(case, side=side, ms=round(r[0], 4), ms_min=round(r[1], 4), ms_max=round(r[2], 4), reps=args.reps, peak_mb=round(peak(fn), 1))
            if bytes_mb is not None:
                ln.update(bytes_mb=round(bytes_mb, 1), of_roof=round(bytes_mb / 1e6 / (r[0] * 1e-3) / ROOF_TBS, 3))
            lines.append(ln)
            print(json.dumps(ln), flush=True)
        verdicts.append(dict(case, speedup=round(res[1][0] / res[0][0], 2), disjoint=bool(res[0][2] < res[1][1] or res[1][2] < res[0][1])))

    def both_modes(case, ring, native, eager, leaves, fwd_bytes, bwd_bytes, eager_leaves=None):
        """native / eager: operand set -> output; leaves (eager_leaves where the eager side has parameters of its own): operand set -> what
        autograd.grad differentiates (the set's last entry is dout)."""
        with torch.no_grad():
            record(dict(case, mode="fwd"), [lambda: native(ring.next()), lambda: eager(ring.next())], fwd_bytes / 1e6)

        def step(fn, lv):
            s = ring.next()
            return torch.autograd.grad(fn(s), lv(s), s[-1])

        record(dict(case, mode="fwd+bwd"), [lambda: step(native, leaves), lambda: step(eager, eager_leaves or leaves)], (fwd_bytes + bwd_bytes) / 1e6)

    def leaf(*shape, dt, scale=1.0, shift=0.0):
        return (torch.randn(*shape, device=dev, dtype=dt) * scale + shift).requires_grad_(True)

    def eager_params(w, b, dt):
        """The eager side's own parameters in the activations' dtype, cast ONCE here, outside every timed call (a module in that dtype
        holds them so); the native side takes the float32 parameters as they are."""
        return w.detach().to(dt).requires_grad_(True), b.detach().to(dt).requires_grad_(True)

    for dt in (torch.float32, torch.float16):
        es = 4 if dt == torch.float32 else 2
        name = str(dt)[6:]
        for B in (1, 5):
            N, C = 8192 * B, 512
            w, b = (t.requires_grad_(True) for t in TR.affine_inputs(C, dev, 1))
            we, be = eager_params(w, b, dt)
            ring = Ring(lambda i: (leaf(N, C, dt=dt, scale=3.0, shift=1.0), torch.randn(N, C, device=dev, dtype=dt)), 2 * N * C * es)
            both_modes(dict(case="layer_norm", shape=[N, C], dtype=name), ring, lambda s: TK.layer_norm(s[0], w, b, EPS),
                       lambda s: F.layer_norm(s[0], (C,), we, be, EPS), lambda s: (s[0], w, b), 2 * N * C * es, 3 * N * C * es,
                       eager_leaves=lambda s: (s[0], we, be))
            del ring
            torch.cuda.empty_cache()
        for Bv in (16, 8):
            N, C = Bv * 4096, 128
            w, b = (t.requires_grad_(True) for t in TR.affine_inputs(C, dev, 2))
            we, be = eager_params(w, b, dt)
            ring = Ring(lambda i: (leaf(N, C, dt=dt), leaf(N, C, dt=dt), torch.randn(N, C, device=dev, dtype=dt), torch.randn(N, C, device=dev, dtype=dt)),
                        4 * N * C * es)

            def eager_tail(s):
                same = (s[1] - s[2]).abs().max() < 1e-6                  # noqa: F841  (the reference's dead test: three launches)
                return s[1] + F.layer_norm(s[0], (C,), we, be, EPS)

            both_modes(dict(case="layer_tail", shape=[N, C], dtype=name), ring, lambda s: TK.layer_norm(s[0], w, b, EPS, residual=s[1]), eager_tail,
                       lambda s: (s[0], s[1], w, b), 3 * N * C * es, 3 * N * C * es, eager_leaves=lambda s: (s[0], s[1], we, be))
            del ring
            torch.cuda.empty_cache()
        for B in (1, 5):
            N, D = 8192 * B, 2048
            ring = Ring(lambda i: (leaf(N, 2 * D, dt=dt), torch.randn(N, D, device=dev, dtype=dt)), 3 * N * D * es)

            def eager_geglu(s):
                h, g = s[0].chunk(2, dim=-1)
                return h * F.gelu(g)

            both_modes(dict(case="geglu", shape=[N, 2 * D], dtype=name), ring, lambda s: TK.geglu(s[0]), eager_geglu, lambda s: (s[0],),
                       3 * N * D * es, 5 * N * D * es)
            del ring
            torch.cuda.empty_cache()

    # one whole stand-in block and layer, patched against unpatched (the same weights)
    def attention(seed):
        a = AR.AttentionStandIn(channels=512, heads=8, seed=seed)
        a.set_processor(DefaultProcessor())
        return a

    blocks = [TR.make_block(512, attention(1), seed=1).to(dev) for _ in range(2)]
    assert TK.use_native_block_ops(blocks[0]) == 3
    xs = Ring(lambda i: leaf(1, 8192, 512, dt=torch.float32), 8192 * 512 * 4)      # (the inputs rotate; the weights are one set, as in use)
    gout = torch.randn(1, 8192, 512, device=dev)

    def nxt():
        return xs.next()

    case = dict(case="block", shape=[1, 8192, 512], dtype="float32")
    with torch.no_grad():
        record(dict(case, mode="fwd"), [lambda: blocks[0](nxt()), lambda: blocks[1](nxt())], None)

    def block_step(m):
        x = nxt()
        return torch.autograd.grad(m(x), [x] + list(m.parameters()), gout)

    record(dict(case, mode="fwd+bwd"), [lambda: block_step(blocks[0]), lambda: block_step(blocks[1])], None)
    layers = [TR.make_layer(128, no_ffn=False, seed=1).to(dev) for _ in range(2)]
    assert TK.use_native_transformer_layers(layers[0]) == 1
    del xs
    torch.cuda.empty_cache()
    xs = Ring(lambda i: leaf(4, 4096, 128, dt=torch.float32), 4 * 4096 * 128 * 4)
    gout = torch.randn(4, 4096, 128, device=dev)
    kw = dict(height=64, width=64, with_shift=False, attn_num_splits=2)
    case = dict(case="layer", shape=[4, 4096, 128], dtype="float32")
    with torch.no_grad():
        record(dict(case, mode="fwd"), [lambda: layers[0](nxt(), nxt(), **kw), lambda: layers[1](nxt(), nxt(), **kw)], None)

    def layer_step(m):
        s, t = nxt(), nxt()
        return torch.autograd.grad(m(s, t, **kw), [s, t] + list(m.parameters()), gout)

    record(dict(case, mode="fwd+bwd"), [lambda: layer_step(layers[0]), lambda: layer_step(layers[1])], None)
    lines.append(dict(case="summary", native_against_eager=verdicts))
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
