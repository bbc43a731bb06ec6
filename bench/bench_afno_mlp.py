"""The AFNO block MLP of the generic route (shapes outside the fused filter's instances): the ``afno_mlp`` kernel against
the route it replaces -- ``models.afno.afno_mlp_aten``: a permuted [nb, M, 2bs] copy, two ``torch.baddbmm`` (hipBLASLt,
fp32), relu and softshrink as separate kernels, and the permute back -- on the same fp32 spectrum windows, hipGraph
timing, the two routes alternated round by round, median of the rounds.

  python bench/bench_afno_mlp.py [--rounds 7] [--out profiles/afno_mlp_r9.txt]

"fp32" rows run the split (bf16x3) weights an fp32 model uses, "bf16" rows the plain bf16 weights a bf16 model uses;
the spectrum is fp32 in both, and the replaced route computes in fp32 for either model.  Every shape is checked
first: both routes against each other.  GB/s is the spectrum read once + written once over the afno_mlp time.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrt_dft_plugins_amd as tdp  # noqa: E402
from bench.bench_fft import time_graph  # noqa: E402
from tensorrt_dft_plugins_amd.models.afno import afno_mlp_aten  # noqa: E402
from tensorrt_dft_plugins_amd.ops import spectral as S  # noqa: E402

# (spectrum window [B, R, km, C, 2], blocks): FourCastNet patch 4 (H = 180), a fraction-0.5 window at embed 768,
# a small AFNO config at block size 32
SHAPES = [((1, 180, 91, 768, 2), 8), ((1, 90, 23, 768, 2), 8), ((8, 32, 17, 256, 2), 8)]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    tdp.load_plugins()
    ops = torch.ops.amd_dft
    dev = "cuda"
    lines = [f"AFNO block MLP on a transformed spectrum, hipGraph, median of {a.rounds} alternated rounds x {a.iters} "
             f"calls [min, max]; us per call, GB/s = (spectrum read + written) / afno_mlp time",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for split in (True, False):
        tag = "fp32" if split else "bf16"
        for shape, nb in SHAPES:
            torch.manual_seed(0)
            C = shape[3]
            bs = C // nb
            xf = torch.randn(*shape, device=dev)
            w1, w2 = (0.05 * torch.randn(2, nb, bs, bs, device=dev) for _ in range(2))
            b1, b2 = (0.05 * torch.randn(2, nb, bs, device=dev) for _ in range(2))
            packed = S.pack_afno_weights(w1, b1, w2, b2, split)
            new = lambda: ops.afno_mlp(xf, *packed, 0.01)  # noqa: E731
            old = lambda: afno_mlp_aten(xf, w1, b1, w2, b2, nb, 0.01).contiguous()  # noqa: E731  (c2r reads it contiguous)
            diff = _rel(new(), old())
            ts = {"aten": [], "afno_mlp": []}
            for _ in range(a.rounds):
                ts["aten"].append(time_graph(old, a.iters))
                ts["afno_mlp"].append(time_graph(new, a.iters))
            o, n = ts["aten"], ts["afno_mlp"]
            mo, mn = statistics.median(o), statistics.median(n)
            tokens = shape[0] * shape[1] * shape[2]
            emit(f"  {tag} {str(list(shape)):<24} bs {bs:<3} aten {mo:8.1f} us [{min(o):.1f}, {max(o):.1f}] | afno_mlp {mn:8.1f} us "
                 f"[{min(n):.1f}, {max(n):.1f}] {2 * xf.numel() * 4 / 1e3 / mn:6.0f} GB/s | aten/afno_mlp {mo / mn:.2f} | "
                 f"rel diff {diff:.1e} | {ops.afno_mlp_info(bs, split, tokens)}")
            del xf
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
