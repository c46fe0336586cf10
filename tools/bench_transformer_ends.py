"""Timing of the native ends of Transformer1D (gnorm.hip through igs_amd.tokens) against the same steps in eager PyTorch, on the same GPU
in the same process, alternating.  One JSON line per case and side:
{"case": "input_end" | "output_end" | "conv", "side": "native" | "eager", "shape", "dtype", "mode": "fwd" | "fwd+bwd", "ms": median of
 HIP-event-timed calls, "ms_min", "ms_max", "reps", "peak_mb", "bytes_mb": the unavoidable bytes (one read of every operand, one write of
 every result), "of_roof": bytes / ms against the measured 6.29 TB/s copy roof}

  input_end   nn.GroupNorm(32, 128, eps 1e-6) over [B, 128, 8192] and the `.permute(0, 2, 1).reshape(...)` copy in front of proj_in
              (igs/models/transformers.py:864-868; the reshape of a permuted tensor copies) against group_norm_tokens
  output_end  `.reshape(...).permute(0, 2, 1).contiguous()` of proj_out's [B, 8192, 128] result, `+ residual`, and the copy that the
              renderer's rearrange "B N D -> (B N) D" makes of GridEncoder.forward's permuted result (transformers.py:899-906) against
              add_residual_tokens and the same permute and reshape, which are views of its token-major buffer
  conv        a stand-in GridEncoder.conv: Transformer1D with 4 blocks of dim 512, 8 heads (use_native_block_ops and use_native_attention on
              both sides) at [1, 128, 8192] float32, without and with use_native_transformer_ends; the downstream permute and rearrange
              copy is counted on the side that has to make it
B = 1 and 5, float32 and float16, forward and forward + backward (autograd.grad to the inputs and parameters).  Every call takes the next of
a ring of operand sets larger than twice the 256 MiB Infinity Cache, so that neither side reads its inputs from it; for the whole module the
inputs rotate through such a ring and the weights are one fixed set per module, as in use.  In float16 the eager GroupNorm gets float16
parameters cast once outside the timed calls and the native side the float32 parameters as they are.  The last line lists, per case, native
against eager: speed-up and whether the min-max ranges are disjoint.

usage: python tools/bench_transformer_ends.py [--reps 20] [--out profiles/transformer_ends_bench.jsonl]
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

ROOF_TBS = 6.29
EPS = 1e-6
C, G, A = 128, 32, 8192


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_transformer_ends needs a GPU"
    import attention_restatement as AR
    import token_ops_restatement as TR
    import transformer_ends_restatement as ER
    from igs_amd import attention as AT, tokens as TK
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
        """native / eager: operand set -> output; leaves: operand set -> what autograd.grad differentiates (the set's last entry is dout)."""
        with torch.no_grad():
            record(dict(case, mode="fwd"), [lambda: native(ring.next()), lambda: eager(ring.next())], fwd_bytes / 1e6)

        def step(fn, lv):
            s = ring.next()
            return torch.autograd.grad(fn(s), lv(s), s[-1])

        record(dict(case, mode="fwd+bwd"), [lambda: step(native, leaves), lambda: step(eager, eager_leaves or leaves)], (fwd_bytes + bwd_bytes) / 1e6)

    def leaf(*shape, dt, scale=1.0, shift=0.0):
        return (torch.randn(*shape, device=dev, dtype=dt) * scale + shift).requires_grad_(True)

    for dt in (torch.float32, torch.float16):
        es = 4 if dt == torch.float32 else 2
        name = str(dt)[6:]
        for B in (1, 5):
            n = B * C * A
            w, b = (t.requires_grad_(True) for t in TR.affine_inputs(C, dev, 1))
            we, be = w.detach().to(dt).requires_grad_(True), b.detach().to(dt).requires_grad_(True)
            ring = Ring(lambda i: (leaf(B, C, A, dt=dt, scale=3.0, shift=1.0), torch.randn(B, A, C, device=dev, dtype=dt)), 2 * n * es)
            both_modes(dict(case="input_end", shape=[B, C, A], dtype=name), ring, lambda s: TK.group_norm_tokens(s[0], G, w, b, EPS),
                       lambda s: F.group_norm(s[0], G, we, be, EPS).permute(0, 2, 1).reshape(B, A, C), lambda s: (s[0], w, b), 2 * n * es, 3 * n * es,
                       eager_leaves=lambda s: (s[0], we, be))
            del ring
            torch.cuda.empty_cache()
            # the set: proj_out's result [B, A, C], the residual [B, C, A], dout for the [(B A), C] rows the interpolation reads
            ring = Ring(lambda i: (leaf(B, A, C, dt=dt), leaf(B, C, A, dt=dt, scale=3.0, shift=1.0), torch.randn(B * A, C, device=dev, dtype=dt)), 3 * n * es)

            def eager_out(s):
                out = s[0].reshape(B, A, C).permute(0, 2, 1).contiguous() + s[1]
                return out.permute(0, 2, 1).reshape(B * A, C)                      # GridEncoder.forward's permute, the renderer's rearrange

            both_modes(dict(case="output_end", shape=[B, C, A], dtype=name), ring,
                       lambda s: TK.add_residual_tokens(s[0], s[1]).permute(0, 2, 1).reshape(B * A, C), eager_out, lambda s: (s[0], s[1]), 3 * n * es, 3 * n * es)
            del ring
            torch.cuda.empty_cache()

    # a stand-in GridEncoder.conv, every other native binder on both sides
    def attention(dim):
        return AR.AttentionStandIn(channels=dim, heads=8, seed=1)

    models = [ER.make_transformer(C, G, 512, 4, seed=1, make_attention=attention).to(dev) for _ in range(2)]
    for m in models:
        assert TK.use_native_block_ops(m) == 12 and AT.use_native_attention(m) == 4
    assert TK.use_native_transformer_ends(models[0]) == 1
    xs = Ring(lambda i: leaf(1, C, A, dt=torch.float32, scale=2.0, shift=0.5), C * A * 4)      # (the inputs rotate; the weights are one set, as in use)
    gout = torch.randn(A, C, device=dev)

    def conv(m):
        return m(xs.next()).permute(0, 2, 1).reshape(A, C)                                     # what interpolate_anchor_features is handed

    case = dict(case="conv", shape=[1, C, A], dtype="float32")
    with torch.no_grad():
        record(dict(case, mode="fwd"), [lambda: conv(models[0]), lambda: conv(models[1])], None)

    def conv_step(m):
        x = xs.next()
        return torch.autograd.grad(m(x).permute(0, 2, 1).reshape(A, C), [x] + list(m.parameters()), gout)

    record(dict(case, mode="fwd+bwd"), [lambda: conv_step(models[0]), lambda: conv_step(models[1])], None)
    lines.append(dict(case="summary", native_against_eager=verdicts))
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
