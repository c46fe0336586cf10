"""Timing of the native swin window attention (wattn.hip through igs_amd.attention.window_attention) against the reference's own sequence
of operations, restated here in PyTorch (roll, split copy, matmul, mask add, softmax, matmul, merge copy, roll back: what
single_head_split_window_attention launches), and, for information, against F.scaled_dot_product_attention with the mask on windows that
were split beforehand (the rolls and the split / merge copies are NOT in that side's time), on the same GPU in the same process,
alternating.  One JSON line per case and side:
{"case", "side": "native" | "restated" | "sdpa_presplit", "B", "dtype", "shift", "ms": median of HIP-event-timed calls, "ms_min", "ms_max",
 "reps", "peak_mb", "tflops", "of_peak"} -- tflops counts the algorithmic work on every side: 4 B h w Lw D per forward (2 products) and
3.5 x that per forward + backward (a backward needs 5 products; the native one executes 7, the float32 one 9: its d K / d V pass owns half
the channels and recomputes S and d P in both halves).  of_peak is against 2500 TF (float16) or 157 TF (float32).

  fwd      B = 8, forward under no_grad (the frozen backbone: 2 B V = 8 images per frame pair at four views)
  fwd_bwd  B = 4, forward + backward to q, k, v (the fine-tuned layer)
h = w = 64, K = 2 (four windows of 1024 tokens per image), D = 128, shifted and not, float32 and float16.
The last line states, for every case, whether the native median is below the restated reference's with disjoint min-max ranges.

usage: python tools/bench_window_attention.py [--reps 20] [--trace] [--out profiles/window_attention_bench.jsonl]
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

from bench_attention import peak, timed_group  # noqa: E402

HW, K, D = 64, 2, 128
PEAK = {torch.float16: 2500.0, torch.float32: 157.0}


def split(t, k):
    b, h, w, c = t.shape
    return t.view(b, k, h // k, k, w // k, c).permute(0, 1, 3, 2, 4, 5).reshape(b * k * k, h // k, w // k, c)


def merge(t, k):
    b, h, w, c = t.shape
    return t.view(b // k // k, k, k, h, w, c).permute(0, 1, 3, 2, 4, 5).contiguous().view(b // k // k, k * h, k * w, c)


def restated(q, k, v, h, w, splits, shift, mask):
    """The reference's sequence of operations (igs/models/unimatch/attention.py:45-104), one PyTorch call per line of it."""
    b, _, c = q.shape
    wh, ww = h // splits, w // splits
    q, k, v = q.view(b, h, w, c), k.view(b, h, w, c), v.view(b, h, w, c)
    if shift:
        q = torch.roll(q, shifts=(-(wh // 2), -(ww // 2)), dims=(1, 2))
        k = torch.roll(k, shifts=(-(wh // 2), -(ww // 2)), dims=(1, 2))
        v = torch.roll(v, shifts=(-(wh // 2), -(ww // 2)), dims=(1, 2))
    q, k, v = split(q, splits), split(k, splits), split(v, splits)
    bn = b * splits * splits
    scores = torch.matmul(q.view(bn, -1, c), k.view(bn, -1, c).permute(0, 2, 1)) / (c ** 0.5)
    if shift:
        scores += mask.repeat(b, 1, 1)
    attn = torch.softmax(scores, dim=-1)
    out = torch.matmul(attn, v.view(bn, -1, c))
    out = merge(out.view(bn, wh, ww, c), splits)
    if shift:
        out = torch.roll(out, shifts=(wh // 2, ww // 2), dims=(1, 2))
    return out.view(b, -1, c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_window_attention needs a GPU"
    import window_attention_restatement as WR
    from igs_amd import attention as AT
    dev = torch.device("cuda:0")
    h = w = HW
    Lw = (h // K) * (w // K)
    lines, verdicts = [], []
    for dt in (torch.float32, torch.float16):
        for shift in (False, True):
            for name, B in (("fwd", 8), ("fwd_bwd", 4)):
                q, k, v, g = WR.random_inputs(B, h, w, dt, dev, seed=B, with_dout=True)
                mask = WR.paint_mask(h, w, K).to(dt).to(dev)
                bw = name == "fwd_bwd"
                if bw:
                    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
                qs, ks, vs = (split(t.detach().view(B, h, w, D), K).reshape(B * K * K, 1, Lw, D).requires_grad_(bw) for t in (q, k, v))
                gs = split(g.view(B, h, w, D), K).reshape(B * K * K, 1, Lw, D)
                ms = mask.repeat(B, 1, 1)[:, None] if shift else None

                def make(side):
                    att = dict(native=lambda: AT.window_attention(q, k, v, h, w, K, shift),
                               restated=lambda: restated(q, k, v, h, w, K, shift, mask),
                               sdpa_presplit=lambda: F.scaled_dot_product_attention(qs, ks, vs, attn_mask=ms))[side]
                    leaves, go = ((qs, ks, vs), gs) if side == "sdpa_presplit" else ((q, k, v), g)

                    def fwd():
                        with torch.no_grad():
                            return att()

                    def fwd_bwd():
                        return torch.autograd.grad(att(), leaves, go)

                    return fwd_bwd if bw else fwd

                if args.trace:
                    fn = make("native")
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    continue
                sides = ["native", "restated", "sdpa_presplit"]
                fns = [make(s) for s in sides]
                res = timed_group(fns, args.reps)
                flop = 4.0 * B * h * w * Lw * D * (3.5 if bw else 1.0)
                case = dict(case=name, B=B, dtype=str(dt).replace("torch.", ""), shift=shift, h=h, w=w, K=K, D=D)
                for side, r, fn in zip(sides, res, fns):
                    ln = dict(case, side=side, ms=round(r[0], 4), ms_min=round(r[1], 4), ms_max=round(r[2], 4), reps=args.reps,
                              peak_mb=round(peak(fn), 1), tflops=round(flop / r[0] / 1e9, 1), of_peak=round(flop / r[0] / 1e9 / PEAK[dt], 4))
                    lines.append(ln)
                    print(json.dumps(ln), flush=True)
                verdicts.append(dict(case=name, B=B, dtype=case["dtype"], shift=shift, against="restated",
                                     ok=bool(res[0][0] < res[1][0] and res[0][2] < res[1][1]), speedup=round(res[1][0] / res[0][0], 2),
                                     sdpa_presplit_speedup=round(res[2][0] / res[0][0], 2)))
                del q, k, v, g, qs, ks, vs, gs, mask, ms
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
