"""Timing of a training step through the residual decoder: forward + backward of the module bound with
use_native_decoder(r, training=True) (mlp.hip: the forward kernel, then igs_mlp_heads_bwd recomputing from x) against the same module's
PyTorch lines under autograd, on the same machine.  Prints one JSON line per case and appends nothing itself: redirect into
profiles/decoder_train_bench.jsonl.  {"case", "n", "dtype", "ms": median over HIP-event-timed calls, "ms_min", "ms_max", "reps", "peak_mb"}.

  train / train_ref       loss = sum of the heads' outputs times fixed gradients; loss.backward() fills x.grad and the ten parameters' .grad
                          (set to None before every call).  Every call of `train` finds the packs cached: the parameters do not change.
  train_kernels           the native launches alone: mlp_heads_fwd + mlp_heads_bwd through the extension, packs given, no autograd
  repack                  pack_mlp(..., transposed=True) alone: what one optimiser step adds to the next native call
Cases: N = 100k and 200k rows; float32, float16, and float32 parameters under float16 autocast ("autocast").
peak_mb: torch.cuda.max_memory_allocated() growth over the call above the operands (x, parameters, upstream gradients), in MB.

usage: python tools/bench_decoder_train.py [--reps 20] [--trace]
"""
import argparse
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from bench_motion import emit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decoder_train needs a GPU"
    import decoder_restatement as DR
    from igs_amd import motion
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for name, dtype, cast in (("float32", torch.float32, False), ("float16", torch.float16, False), ("autocast", torch.float32, True)):
        ref = DR.make_renderer(dim_in=128, n_neurons=128, dim_out=128, n_hidden_layers=2, seed=1).to(dev).to(dtype)
        nat = DR.make_renderer(dim_in=128, n_neurons=128, dim_out=128, n_hidden_layers=2, seed=1).to(dev).to(dtype)
        motion.use_native_decoder(nat, training=True)
        ctx = (lambda: torch.autocast("cuda", dtype=torch.float16)) if cast else contextlib.nullcontext
        for n in (100000, 200000):
            x = torch.randn(n, 128, generator=g).to(dtype).to(dev).requires_grad_(True)
            douts = [torch.randn(n, ch, generator=g).to(dev) for ch in (3, 4)]

            def step(r):
                x.grad = None
                r.zero_grad(set_to_none=True)
                with ctx():
                    d = r.decode_residual_feature(x)
                torch.autograd.backward(list(d.values()), [gk.to(v.dtype) for gk, v in zip(douts, d.values())])
            case = dict(n=n, dtype=name)
            emit(args, lambda: step(nat), case="train", **case)
            emit(args, lambda: step(ref), case="train_ref", **case)
            lin = [m for m in nat.mlp_net.layers if isinstance(m, torch.nn.Linear)]
            parts = ([m.weight for m in lin], [m.bias for m in lin], [m.weight for m in nat.out_layers], [m.bias for m in nat.out_layers])
            kd = torch.float16 if cast else dtype
            wpack, bpack, wpack_t = motion.pack_mlp(*parts, transposed=True, dtype=kd)
            xk, gk, E = x.detach().to(kd), [t.to(kd) for t in douts], motion._ext()._mlp

            def kernels():
                E.mlp_heads_fwd(xk, wpack, bpack, [128] * 4, [1, 1, 0], [3, 4], 0)
                E.mlp_heads_bwd(xk, wpack, wpack_t, bpack, [128] * 4, [1, 1, 0], [3, 4], 0, gk, True, True, True)
            emit(args, kernels, case="train_kernels", **case)
            emit(args, lambda: motion.pack_mlp(*parts, transposed=True, dtype=kd), case="repack", **case)
            del x, douts, xk, gk


if __name__ == "__main__":
    main()
