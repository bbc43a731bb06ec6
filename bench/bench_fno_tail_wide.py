"""The FNO layer tail above 32 channels at 720x1440 (B = 1, m = 32): the wide fused kernel (fno_c2r_pw / fno_c2r as
routed) against the split route it replaces, written out here as its two ops -- c2r along W (writes the
full-resolution spectral output) followed by fno_pointwise (reads it back) -- bf16 and fp32, hipGraph timing, the
two routes alternated round by round, median of the rounds.  Also a whole FNOBlock at width 64 (amd backend).

  python bench/bench_fno_tail_wide.py [--rounds 7] [--out profiles/fno_tail_wide_r8.txt]

Every shape is checked first: the two routes against each other.  GB/s is the fused route's traffic (x and y once,
y only for fno_c2r) over the measured time.  In a tuning build (csrc/ops/tuning.h) MI_DFT_FNO_WIDE=0 sends the ops
themselves down the split route; this script does not need one.
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
from tensorrt_dft_plugins_amd.models.fno import FNOBlock  # noqa: E402

H, W, M = 720, 1440, 32
PW_SHAPES = [(64, 64), (128, 128), (40, 40)]
C2R_SHAPES = [64, 128]


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
    lines = [f"FNO layer tail, B=1, {H}x{W}, m={M}, hipGraph, median of {a.rounds} alternated rounds x {a.iters} calls "
             f"[min, max]; us per call, GB/s = (x + y bytes) / time of the fused route",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    def run(fns):
        ts = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ts[k].append(time_graph(fn, a.iters))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}

    def row(tag, name, info, r, gb, diff):
        f, s = r["fused"], r["split"]
        emit(f"  {tag} {name:<22} split {s[0]:8.1f} us [{s[1]:.1f}, {s[2]:.1f}] | fused {f[0]:8.1f} us [{f[1]:.1f}, {f[2]:.1f}] "
             f"{gb / f[0]:6.0f} GB/s | split/fused {s[0] / f[0]:.2f} | rel diff {diff:.1e} | {info}")

    emit("A. fno_c2r_pw (irfft_W + conv1x1 + bias + GELU): c2r + fno_pointwise vs the fused route")
    for dt in (torch.bfloat16, torch.float32):
        tag = "bf16" if dt == torch.bfloat16 else "fp32"
        es = 2 if dt == torch.bfloat16 else 4
        for ci, co in PW_SHAPES:
            torch.manual_seed(0)
            yw = torch.randn(1, co, H, M, 2, device=dev) / (2 * M) ** 0.5
            x = torch.randn(1, ci, H, W, device=dev).to(dt)
            w = torch.randn(co, ci, device=dev) / ci ** 0.5
            b = torch.randn(co, device=dev)
            fused = lambda: ops.fno_c2r_pw(yw, x, w, b, True)  # noqa: E731
            split = lambda: ops.fno_pointwise(ops.c2r(yw, [3], [W], 1.0, [], dt), x, w, b, True)  # noqa: E731
            diff = _rel(fused().float(), split().float())
            r = run({"split": split, "fused": fused})
            row(tag, f"{ci:>3} -> {co:<3}", ops.fno_c2r_pw_info(ci, co, M, W, dt == torch.bfloat16), r,
                (ci + co) * H * W * es / 1e3, diff)
            del yw, x
            torch.cuda.empty_cache()
    emit("")
    emit("B. fno_c2r (irfft_W only): c2r vs the fused route")
    for dt in (torch.bfloat16, torch.float32):
        tag = "bf16" if dt == torch.bfloat16 else "fp32"
        es = 2 if dt == torch.bfloat16 else 4
        for co in C2R_SHAPES:
            torch.manual_seed(0)
            yw = torch.randn(1, co, H, M, 2, device=dev) / (2 * M) ** 0.5
            fused = lambda: ops.fno_c2r(yw, W, dt)  # noqa: E731
            split = lambda: ops.c2r(yw, [3], [W], 1.0, [], dt)  # noqa: E731
            diff = _rel(fused().float(), split().float())
            r = run({"split": split, "fused": fused})
            row(tag, f"fno_c2r {co:<3}", ops.fno_c2r_pw_info(0, co, M, W, dt == torch.bfloat16), r, co * H * W * es / 1e3,
                diff)
            del yw
            torch.cuda.empty_cache()
    emit("")
    emit("C. FNOBlock width 64, modes 32 x 32 (amd backend, as routed)")
    for dt in (torch.bfloat16, torch.float32):
        tag = "bf16" if dt == torch.bfloat16 else "fp32"
        torch.manual_seed(0)
        blk = FNOBlock(64, 32, 32, backend="amd").to(dev).eval()
        x = torch.randn(1, 64, H, W, device=dev).to(dt)
        with torch.no_grad():
            fn = lambda: blk(x)  # noqa: E731
            ts = [time_graph(fn, a.iters) for _ in range(a.rounds)]
        emit(f"  {tag} FNOBlock 64  {statistics.median(ts):8.1f} us [{min(ts):.1f}, {max(ts):.1f}]")
        del x, blk
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
