"""Timing of the native fused attention (attn.hip through igs_amd.attention) against F.scaled_dot_product_attention as PyTorch dispatches
it (what diffusers' default processor calls) and against the same call under SDPBackend.MATH, on the same GPU in the same process,
alternating.  One JSON line per case and side:
{"case", "side": "native" | "sdpa" | "math", "B", "dtype", "ms": median of HIP-event-timed calls, "ms_min", "ms_max", "reps", "peak_mb",
 "tflops", "of_peak"} -- tflops counts the algorithmic work on every side: 4 B H A^2 D per forward (2 products) and 3.5 x that per forward +
backward (a backward needs 5 products).  The native backward recomputes S and d P in both of its passes, 7 products, so its matrix units
do 9 / 7 of the counted work per forward + backward.  of_peak is against 2500 TF (float16) or 157 TF (float32).

  fwd        forward under no_grad, q / k / v [B, 8, 8192, 64] head-major on every side
  fwd_bwd    forward + backward to q, k, v
  block      one Transformer1D-shaped block end to end (LayerNorm, attention with the processor, LayerNorm, GEGLU feed-forward, residuals)
  block_bwd  on [B, 8192, 512], forward and forward + backward to the input and all weights; the reference side is the same block with
             the default processor's calls (head split by view + transpose, F.scaled_dot_product_attention, transpose back)
The last line states, for every case, whether the native median is below the reference's with disjoint min-max ranges.

usage: python tools/bench_attention.py [--reps 20] [--trace] [--out profiles/attention_bench.jsonl]
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

H, A, D = 8, 8192, 64
PEAK = {torch.float16: 2500.0, torch.float32: 157.0}


def timed_group(fns, reps, warmup=2):
    """[(median, min, max)] of every function, timed alternately."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
    out = []
    for t in ts:
        t.sort()
        out.append((t[len(t) // 2], t[0], t[-1]))
    return out


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    del r
    return (torch.cuda.max_memory_allocated() - base) / 1e6


class DefaultProcessor:
    """The calls of diffusers' default (PyTorch 2) attention processor on a [B, A, C] input."""

    def __init__(self, math=False):
        self.math = math

    def __call__(self, attn, x, encoder_hidden_states=None, attention_mask=None, temb=None, **kw):
        B, A_, C = x.shape
        sp = lambda t: t.view(B, A_, attn.heads, C // attn.heads).transpose(1, 2)
        q, k, v = sp(attn.to_q(x)), sp(attn.to_k(x)), sp(attn.to_v(x))
        if self.math:
            from torch.nn.attention import SDPBackend, sdpa_kernel
            with sdpa_kernel(SDPBackend.MATH):
                o = F.scaled_dot_product_attention(q, k, v, scale=attn.scale)
        else:
            o = F.scaled_dot_product_attention(q, k, v, scale=attn.scale)
        o = o.transpose(1, 2).reshape(B, A_, C)
        return attn.to_out[1](attn.to_out[0](o))


class Block(torch.nn.Module):
    """BasicTransformerBlock as Transformer1D configures it: norm1, self-attention, residual, norm3, GEGLU feed-forward, residual."""

    def __init__(self, attn, C=512):
        super().__init__()
        self.norm1, self.attn1, self.norm3 = torch.nn.LayerNorm(C), attn, torch.nn.LayerNorm(C)
        self.proj, self.out = torch.nn.Linear(C, 8 * C), torch.nn.Linear(4 * C, C)

    def forward(self, x):
        x = x + self.attn1(self.norm1(x))
        h, gate = self.proj(self.norm3(x)).chunk(2, -1)
        return x + self.out(h * F.gelu(gate))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_attention needs a GPU"
    import attention_restatement as AR
    from igs_amd import attention as AT
    from torch.nn.attention import SDPBackend, sdpa_kernel
    dev = torch.device("cuda:0")
    scale = D ** -0.5
    lines, verdicts = [], []
    for B in (1, 5):
        for dt in (torch.float32, torch.float16):
            q, k, v, g = AR.random_inputs(B, H, A, A, dt, dev, seed=B, with_dout=True)
            qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
            x = torch.randn(B, A, H * D, device=dev, dtype=dt)
            xg = x.clone().requires_grad_(True)
            gx = torch.randn(B, A, H * D, device=dev, dtype=dt)
            blocks = {}
            for side in ("native", "sdpa", "math"):
                attn = AR.AttentionStandIn(seed=1)
                attn.set_processor(AT.AnchorAttnProcessor() if side == "native" else DefaultProcessor(math=side == "math"))
                torch.manual_seed(2)
                blocks[side] = Block(attn).to(dev).to(dt)

            def math_call(fn):
                def run():
                    with sdpa_kernel(SDPBackend.MATH):
                        return fn()
                return run

            def make(side, case):
                att = dict(native=lambda a, b, c: AT.sdpa(a, b, c, scale=scale),
                           sdpa=lambda a, b, c: F.scaled_dot_product_attention(a, b, c, scale=scale),
                           math=lambda a, b, c: F.scaled_dot_product_attention(a, b, c, scale=scale))[side]
                blk = blocks[side]
                params = list(blk.parameters())

                def fwd():
                    with torch.no_grad():
                        return att(q, k, v)

                def fwd_bwd():
                    return torch.autograd.grad(att(qg, kg, vg), (qg, kg, vg), g)

                def block():
                    with torch.no_grad():
                        return blk(x)

                def block_bwd():
                    return torch.autograd.grad(blk(xg), [xg] + params, gx)

                fn = dict(fwd=fwd, fwd_bwd=fwd_bwd, block=block, block_bwd=block_bwd)[case]
                return math_call(fn) if side == "math" and case in ("fwd", "fwd_bwd") else fn

            if args.trace:
                for c in ("fwd", "fwd_bwd", "block", "block_bwd"):
                    fn = make("native", c)
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                continue
            case = dict(B=B, dtype=str(dt).replace("torch.", ""), H=H, A=A, D=D)
            sides = ["native", "sdpa", "math"]
            for name in ("fwd", "fwd_bwd", "block", "block_bwd"):
                fns = [make(s, name) for s in sides]
                res = timed_group(fns, args.reps)
                flop = 4.0 * B * H * A * A * D * (3.5 if name.endswith("bwd") else 1.0)
                for side, r, fn in zip(sides, res, fns):
                    ln = dict(case, case=name, side=side, ms=round(r[0], 4), ms_min=round(r[1], 4), ms_max=round(r[2], 4), reps=args.reps,
                              peak_mb=round(peak(fn), 1))
                    if name in ("fwd", "fwd_bwd"):
                        ln["tflops"] = round(flop / r[0] / 1e9, 1)
                        ln["of_peak"] = round(flop / r[0] / 1e9 / PEAK[dt], 4)
                    lines.append(ln)
                    print(json.dumps(ln), flush=True)
                for i, ref in enumerate(sides[1:], 1):
                    verdicts.append(dict(case=name, B=B, dtype=case["dtype"], against=ref, ok=bool(res[0][0] < res[i][0] and res[0][2] < res[i][1]),
                                         speedup=round(res[i][0] / res[0][0], 2)))
            del q, k, v, g, qg, kg, vg, x, xg, gx, blocks
            torch.cuda.empty_cache()
    if not args.trace:
        lines.append(dict(case="merge_condition", holds=all(v["ok"] for v in verdicts), cases=verdicts))
        print(json.dumps(lines[-1]), flush=True)
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
