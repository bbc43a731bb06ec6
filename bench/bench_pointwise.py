"""fno_pointwise at 720x1440: the register-resident instances against the MFMA kernel, and the MFMA kernel against
eager torch (conv2d + add + gelu), bf16 and fp32, hipGraph timing, the variants alternated round by round.

The fixed-vs-MFMA comparison needs a tuning build (csrc/ops/tuning.h): MI_DFT_PW_MFMA=1 routes the seven fixed
channel counts to the MFMA kernel, read by the route function at every call:

  MI_DFT_HIPCC_EXTRA=-DAMD_DFT_TUNING=1 python -m tensorrt_dft_plugins_amd._build --out variants/tuning
  MI_DFT_LIB=variants/tuning/_C.so python bench/bench_pointwise.py [--rounds 7] [--out profiles/fno_pointwise_mfma_r7.txt]

Every shape is checked first: both kernels against each other (fixed vs MFMA) or against the eager result.
GB/s is the algorithm's traffic (x, spec and y once) over the measured time.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrt_dft_plugins_amd as tdp  # noqa: E402
from bench.bench_fft import time_graph  # noqa: E402

H, W = 720, 1440
AB_SHAPES = [(20, 128), (128, 20), (64, 64), (64, 256)]   # fixed instance vs MFMA (tuning build)
EAGER_SHAPES = [(3, 32), (12, 40), (40, 40)]               # MFMA vs eager torch


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
    tuning = bool(ops.tuning_build())
    dev = "cuda"
    lines = [f"fno_pointwise (spec + conv1x1 + bias + GELU), B=1, {H}x{W}, hipGraph, median of {a.rounds} alternated "
             f"rounds x {a.iters} calls; us per call, GB/s = (x + spec + y bytes) / time",
             f"device: {torch.cuda.get_device_name(0)}; tuning build: {tuning}", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    def run(fns):
        ts = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ts[k].append(time_graph(fn, a.iters))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}

    def mfma(on):
        os.environ["MI_DFT_PW_MFMA"] = "1" if on else "0"

    emit("A. fixed instance vs MFMA kernel" + ("" if tuning else "  -- SKIPPED: needs a tuning build (MI_DFT_LIB)"))
    for dt in (torch.bfloat16, torch.float32):
        tag = "bf16" if dt == torch.bfloat16 else "fp32"
        es = 2 if dt == torch.bfloat16 else 4
        for ci, co in AB_SHAPES if tuning else []:
            torch.manual_seed(0)
            x = torch.randn(1, ci, H, W, device=dev).to(dt)
            s = torch.randn(1, co, H, W, device=dev).to(dt)
            w = torch.randn(co, ci, device=dev) / ci ** 0.5
            b = torch.randn(co, device=dev)
            call = lambda: ops.fno_pointwise(s, x, w, b, True)  # noqa: E731
            mfma(False)
            yf = call()
            mfma(True)
            ym = call()
            diff = _rel(ym.float(), yf.float())

            def fixed_fn():
                mfma(False)
                call()

            def mfma_fn():
                mfma(True)
                call()

            r = run({"fixed": fixed_fn, "mfma": mfma_fn})
            mfma(False)
            gb = (ci + 2 * co) * H * W * es / 1e3
            emit(f"  {tag} {ci:>3} -> {co:<3}  fixed {r['fixed'][0]:8.1f} us [{r['fixed'][1]:.1f}, {r['fixed'][2]:.1f}] "
                 f"{gb / r['fixed'][0]:6.0f} GB/s | mfma {r['mfma'][0]:8.1f} us [{r['mfma'][1]:.1f}, {r['mfma'][2]:.1f}] "
                 f"{gb / r['mfma'][0]:6.0f} GB/s | mfma/fixed {r['mfma'][0] / r['fixed'][0]:.2f} | rel diff {diff:.1e}")
            del x, s, yf, ym
            torch.cuda.empty_cache()
    emit("")
    emit("B. MFMA kernel vs eager torch (conv2d + add + gelu)")
    for dt in (torch.bfloat16, torch.float32):
        tag = "bf16" if dt == torch.bfloat16 else "fp32"
        es = 2 if dt == torch.bfloat16 else 4
        for ci, co in EAGER_SHAPES:
            assert ops.fno_pointwise_info(ci, co, dt == torch.bfloat16, H * W).startswith("mfma")
            torch.manual_seed(0)
            x = torch.randn(1, ci, H, W, device=dev).to(dt)
            s = torch.randn(1, co, H, W, device=dev).to(dt)
            w = torch.randn(co, ci, device=dev) / ci ** 0.5
            b = torch.randn(co, device=dev)
            w4, bt = w.to(dt)[:, :, None, None].contiguous(), b.to(dt)
            eager = lambda: F.gelu(F.conv2d(x, w4, bt) + s)  # noqa: E731
            hand = lambda: ops.fno_pointwise(s, x, w, b, True)  # noqa: E731
            diff = _rel(hand().float(), eager().float())
            r = run({"eager": eager, "mfma": hand})
            gb = (ci + 2 * co) * H * W * es / 1e3
            verdict = "MFMA LOSES to eager torch" if r["mfma"][0] > r["eager"][0] else "mfma faster"
            emit(f"  {tag} {ci:>3} -> {co:<3}  eager {r['eager'][0]:8.1f} us [{r['eager'][1]:.1f}, {r['eager'][2]:.1f}] | "
                 f"mfma {r['mfma'][0]:8.1f} us [{r['mfma'][1]:.1f}, {r['mfma'][2]:.1f}] {gb / r['mfma'][0]:6.0f} GB/s | "
                 f"eager/mfma {r['eager'][0] / r['mfma'][0]:.2f} ({verdict}) | rel diff {diff:.1e}")
            del x, s
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
