"""Timing of the fused residual decoder (mlp.hip through igs_amd.motion) against the same lines in eager PyTorch on the same machine.
Prints one JSON line per case: {"case", "n", "dtype", "ms": median over HIP-event-timed calls, "ms_min", "ms_max", "reps", "peak_mb",
"hbm_floor_ms", "matrix_floor_ms"}.

  decoder / decoder_ref   the shipped decoder (configs/train.yaml:205-217: Linear(128,128) SiLU Linear(128,128) SiLU Linear(128,128), then
                          Linear(128,3) and Linear(128,4)) under no_grad: the bound module's one launch vs a stand-in nn.Sequential plus
                          heads (gs.py:858-869's lines: 5 GEMM and 2 activation launches)
  decoder_kernel_x8       eight launches of the kernel alone per timed call (packed weights, no Python layer): ms / 8 is one kernel's time
Cases: N = 100k and 200k rows, float32 and float16.
Budgets, printed next to the results: hbm_floor_ms = N (128 + 7) elements / 6.3 TB/s (the achievable HBM rate; float32: N (512 + 28) B);
matrix_floor_ms = 2 N (3 * 128^2 + 128 * 32) FLOP / 155 TFLOP/s (f32 MFMA, measured) or / 2.5 PFLOP/s (f16 MFMA, dense spec): the heads
occupy one 32-wide tile.
peak_mb: torch.cuda.max_memory_allocated() growth over the call, in MB.

usage: python tools/bench_decoder.py [--reps 20] [--trace]
  --trace: 3 calls per case and no timing lines (for a rocprofv3 --kernel-trace --stats run)
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

from bench_motion import emit  # noqa: E402

HBM_BYTES_PER_S, F32_FLOPS, F16_FLOPS = 6.3e12, 155e12, 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decoder needs a GPU"
    import decoder_restatement as DR
    from igs_amd import motion
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.float32, torch.float16):
        ref = DR.make_renderer(dim_in=128, n_neurons=128, dim_out=128, n_hidden_layers=2, seed=1).to(dev).to(dtype).eval()
        nat = DR.make_renderer(dim_in=128, n_neurons=128, dim_out=128, n_hidden_layers=2, seed=1).to(dev).to(dtype).eval()
        motion.use_native_decoder(nat)
        es = 4 if dtype == torch.float32 else 2
        for n in (100000, 200000):
            x = torch.randn(n, 128, generator=g).to(dtype).to(dev)
            case = dict(n=n, dtype=str(dtype).split(".")[1], hbm_floor_ms=round(n * 135 * es / HBM_BYTES_PER_S * 1e3, 4),
                        matrix_floor_ms=round(2 * n * (3 * 128 * 128 + 128 * 32) / (F32_FLOPS if es == 4 else F16_FLOPS) * 1e3, 4))
            with torch.no_grad():
                emit(args, lambda: nat.decode_residual_feature(x), case="decoder", **case)
                emit(args, lambda: ref.decode_residual_feature(x), case="decoder_ref", **case)
                # the launch alone, 8 in a row per timed call so that the host's share of a call is hidden behind the kernels: ms / 8 is one kernel
                (wpack, bpack), E = vars(nat)[motion.DECODER_CACHE]["pack"], motion._ext()._mlp
                emit(args, lambda: [E.mlp_heads_fwd(x, wpack, bpack, [128] * 4, [1, 1, 0], [3, 4], 0) for _ in range(8)], case="decoder_kernel_x8", **case)
            del x


if __name__ == "__main__":
    main()
