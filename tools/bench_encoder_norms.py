"""Timing of the native encoder norms and position add (inorm.hip through igs_amd.backbone) against the same steps in eager PyTorch
(F.instance_norm, relu_, add, relu; the reference's feature_add_position restated from its split / embedding / merge operations), on the
same GPU in the same process, alternating.  One JSON line per case and side:
{"case": "norm" | "position" | "encoder", "side": "native" | "eager" | ..., "shape", "dtype", "mode", "ms": median of HIP-event-timed calls,
 "ms_min", "ms_max", "reps", "peak_mb", "bytes_mb": the unavoidable bytes (one read of every operand, one write of the result),
 "of_roof": bytes / ms against the measured 6.29 TB/s copy roof}

  norm      [8, 64, 256, 256], [8, 96, 128, 128], [8, 128, 64, 64] x float32, float16 x the four modes, out of place on both sides
  position  feature_add_position at [8, 128, 64, 64], K = 2
  encoder   one whole forward of the stand-in encoder of tests/encoder_norms_restatement.py at [8, 3, 512, 512] float32: unpatched,
            patched with use_native_encoder_norms, and with every norm replaced by nn.Identity (the convolutions, ReLUs and adds alone)
Every call takes the next of a ring of operand sets larger than twice the 256 MiB Infinity Cache, so that neither side reads its inputs from it.
The last line lists, per case, native against eager: speed-up and whether the min-max ranges are disjoint.

usage: python tools/bench_encoder_norms.py [--reps 20] [--out profiles/encoder_norms_bench.jsonl]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_attention import peak, timed_group  # noqa: E402

ROOF_TBS = 6.29
SHAPES = ((8, 64, 256, 256), (8, 96, 128, 128), (8, 128, 64, 64))
MODE_NAMES = ("PLAIN", "RELU", "RELU_ADD_RELU", "RELU_ADDNORM_RELU")
RING_BYTES = 600e6


def eager_mode(x, skip, mode, eps=1e-5):
    """The reference's own calls for the mode (igs/models/unimatch/backbone.py:30-36)."""
    y = F.instance_norm(x, eps=eps)
    if mode == 0:
        return y
    y = torch.relu_(y)
    if mode == 1:
        return y
    if mode == 3:
        skip = F.instance_norm(skip, eps=eps)
    return torch.relu_(skip + y)


def eager_position(f0, f1, K):
    """feature_add_position as the reference launches it: split both, build the sine embedding of the window, add, merge both."""
    def split(t):
        b, c, h, w = t.shape
        return t.view(b, c, K, h // K, K, w // K).permute(0, 2, 4, 1, 3, 5).reshape(b * K * K, c, h // K, w // K)

    def merge(t, b):
        _, c, h, w = t.shape
        return t.view(b, K, K, c, h, w).permute(0, 3, 1, 4, 2, 5).contiguous().view(b, c, K * h, K * w)

    b, c = f0.shape[:2]
    s0, s1 = split(f0), split(f1)
    n = c // 2
    mask = torch.ones((s0.shape[0], s0.shape[2], s0.shape[3]), device=f0.device)
    ye, xe = mask.cumsum(1, dtype=torch.float32), mask.cumsum(2, dtype=torch.float32)
    ye = ye / (ye[:, -1:, :] + 1e-6) * (2 * math.pi)
    xe = xe / (xe[:, :, -1:] + 1e-6) * (2 * math.pi)
    dim = torch.arange(n, dtype=torch.float32, device=f0.device)
    dim = 10000 ** (2 * (dim // 2) / n)
    px, py = xe[:, :, :, None] / dim, ye[:, :, :, None] / dim
    px = torch.stack((px[:, :, :, 0::2].sin(), px[:, :, :, 1::2].cos()), dim=4).flatten(3)
    py = torch.stack((py[:, :, :, 0::2].sin(), py[:, :, :, 1::2].cos()), dim=4).flatten(3)
    pos = torch.cat((py, px), dim=3).permute(0, 3, 1, 2).to(f0.dtype)
    return merge(s0 + pos, b), merge(s1 + pos, b)


class Ring:
    """Operand sets handed out in turn."""

    def __init__(self, make, bytes_per_set):
        self.sets = [make(i) for i in range(max(3, int(math.ceil(RING_BYTES / bytes_per_set))))]
        self.i = 0

    def next(self):
        self.i = (self.i + 1) % len(self.sets)
        return self.sets[self.i]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_encoder_norms needs a GPU"
    import encoder_norms_restatement as ER
    from igs_amd import backbone as BB
    dev = torch.device("cuda:0")
    lines, verdicts = [], []

    def record(case, sides, fns, bytes_mb):
        res = timed_group(fns, args.reps)
        for side, r, fn in zip(sides, res, fns):
            ln = dict(case, side=side, ms=round(r[0], 4), ms_min=round(r[1], 4), ms_max=round(r[2], 4), reps=args.reps, peak_mb=round(peak(fn), 1))
            if bytes_mb is not None:
                ln.update(bytes_mb=round(bytes_mb, 1), of_roof=round(bytes_mb / 1e6 / (r[0] * 1e-3) / ROOF_TBS, 3))
            lines.append(ln)
            print(json.dumps(ln), flush=True)
        verdicts.append(dict(case, speedup=round(res[1][0] / res[0][0], 2), disjoint=bool(res[0][2] < res[1][1] or res[1][2] < res[0][1])))
        return res

    with torch.no_grad():
        for shape in SHAPES:
            for dt in (torch.float32, torch.float16):
                nbytes = math.prod(shape) * (4 if dt == torch.float32 else 2)
                ring = Ring(lambda i: (torch.randn(shape, device=dev, dtype=dt) * 3 + 1, torch.randn(shape, device=dev, dtype=dt)), 2 * nbytes)
                for mode in range(4):
                    def native():
                        x, k = ring.next()
                        if mode >= 2:
                            return BB.residual_tail(x, k, norm_skip=mode == 3)
                        return BB.instance_norm(x, relu=mode == 1)

                    def eager():
                        x, k = ring.next()
                        return eager_mode(x, k, mode)

                    record(dict(case="norm", shape=list(shape), dtype=str(dt)[6:], mode=MODE_NAMES[mode]), ["native", "eager"], [native, eager],
                           nbytes * (3 if mode >= 2 else 2) / 1e6)
                del ring
                torch.cuda.empty_cache()
        shape = (8, 128, 64, 64)
        for dt in (torch.float32, torch.float16):
            nbytes = math.prod(shape) * (4 if dt == torch.float32 else 2)
            ring = Ring(lambda i: (torch.randn(shape, device=dev, dtype=dt), torch.randn(shape, device=dev, dtype=dt)), 2 * nbytes)
            record(dict(case="position", shape=list(shape), dtype=str(dt)[6:], mode="K=2"), ["native", "eager"],
                   [lambda: BB.feature_add_position(*ring.next(), 2, 128), lambda: eager_position(*ring.next(), 2)], 4 * nbytes / 1e6)
            del ring
            torch.cuda.empty_cache()
        # the whole stand-in encoder
        imgs = [torch.randn(8, 3, 512, 512, device=dev) for _ in range(3)]
        turn = [0]

        def img():
            turn[0] = (turn[0] + 1) % len(imgs)
            return imgs[turn[0]]

        eager_enc = ER.make_encoder(seed=1).to(dev)
        native_enc = ER.make_encoder(seed=1).to(dev)
        assert BB.use_native_encoder_norms(native_enc) == 15
        conv_enc = ER.make_encoder(seed=1, norm=lambda c: nn.Identity()).to(dev)
        record(dict(case="encoder", shape=[8, 3, 512, 512], dtype="float32", mode="forward"), ["native", "eager", "identity_norms"],
               [lambda: native_enc(img()), lambda: eager_enc(img()), lambda: conv_enc(img())], None)
    lines.append(dict(case="summary", native_against_eager=verdicts))
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
