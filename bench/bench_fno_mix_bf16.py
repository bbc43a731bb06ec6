"""The bf16 ``fno_mix`` kernels against the fp32 op on the same operands (rounded to bf16), and -- where the weights
have a per-degree form -- against the bf16 ``sfno_mix`` on that form; then a small bf16 ``SFNOBlock`` under
``mix="degree"`` and ``mix="expand"``.  hipGraph timing, the routes alternated round by round in one process, the median
of the rounds with [min, max] (the method of bench_sfno_mix.py).

  python bench/bench_fno_mix_bf16.py [--rounds 7] [--out profiles/fno_mix_bf16_r14.txt]

(bench/bench_fno_mix.py is the FNO block under its two mode-mixing paths; this file times the op.)
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrt_dft_plugins_amd as tdp  # noqa: E402
from bench.bench_sfno_mix import _fmt, _rel, _timed  # noqa: E402
from tensorrt_dft_plugins_amd.models import sfno  # noqa: E402
from tensorrt_dft_plugins_amd.ops import spectral as SP  # noqa: E402

# (B, C = Cin = Cout, modes, (L, M) of the per-degree form or None)
SHAPES = [(1, 20, 64 * 64, (64, 64)), (8, 20, 2048, None), (32, 20, 2048, None), (4, 64, 128 * 128, (128, 128))]
SMALL_BLOCK = (1, 20, 64, 128)
GRID = "equiangular"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    tdp.load_plugins()
    ops = torch.ops.amd_dft
    dev, bf = "cuda", torch.bfloat16
    lines = [f"fno_mix, bf16 against fp32 of the same op on the same (bf16-valued) operands, hipGraph, median of {a.rounds} "
             f"alternated rounds x {a.iters} calls [min, max]; us per call; sfno_mix = the bf16 per-degree kernel on the "
             "per-degree weights (tri = 1), where the weights are an expansion of them",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    with torch.no_grad():
        for B, C, modes, degree in SHAPES:
            torch.manual_seed(0)
            if degree:
                L, M = degree
                c16 = tdp.sht(torch.randn(B, C, L, 2 * M, device=dev), L, M, GRID).to(bf)  # zero where l < m
                wd16 = (torch.rand(C, C, L, 2, device=dev) / (C * C)).to(bf)
                w16 = wd16[:, :, :, None, :].expand(-1, -1, -1, M, -1).reshape(C, C, L * M, 2).contiguous()
                x16 = c16.reshape(B, C, L * M, 2)
            else:
                x16 = torch.randn(B, C, modes, 2, device=dev).to(bf)
                w16 = (torch.rand(C, C, modes, 2, device=dev) / (C * C)).to(bf)
            x32, w32 = x16.float(), w16.float()
            routes = [("fp32", lambda: ops.fno_mix(x32, w32, 0)), ("bf16", lambda: ops.fno_mix(x16, w16, 0))]
            diffs = [f"bf16 vs fp32 {_rel(routes[1][1](), routes[0][1]()):.1e}"]
            if degree:
                ws16 = SP.sfno_mix_split(wd16)
                routes.append(("sfno_mix", lambda: ops.sfno_mix(c16, wd16, ws16, 1)))
                diffs.append(f"sfno_mix vs fp32 {_rel(routes[2][1]().reshape(B, C, L * M, 2), routes[0][1]()):.1e}")
            emit(f"[{B}, {C}, {modes}]  weights {w16.numel() * 2 / 2 ** 20:.1f} MiB (fp32: {w32.numel() * 4 / 2 ** 20:.1f})   "
                 f"fp32: {ops.fno_mix_info(B, C, C, modes)}   bf16: {ops.fno_mix_info(B, C, C, modes, True)}")
            t = _timed(routes, a.rounds, a.iters)
            med = {k: statistics.median(v) for k, v in t.items()}
            row = "  " + " | ".join(_fmt(name, t[name]) for name, _ in routes) + f" | fp32/bf16 {med['fp32'] / med['bf16']:.2f}"
            if degree:
                row += f" | sfno_mix/bf16 {med['sfno_mix'] / med['bf16']:.2f}"
            emit(row + " | rel diff " + ", ".join(diffs))
            del x16, x32, w16, w32, routes
            torch.cuda.empty_cache()

        B, C, nlat, nlon = SMALL_BLOCK
        torch.manual_seed(0)
        x = torch.randn(B, C, nlat, nlon, device=dev).to(bf)
        blk = sfno.SFNOBlock(C, nlat, nlon, grid=GRID, backend="amd", mix="degree").to(dev).eval()

        def run(mix):
            blk.spectral.mix = mix
            return blk(x)

        diff = _rel(run("expand"), run("degree"))
        t = _timed([("degree", lambda: run("degree")), ("expand", lambda: run("expand"))], a.rounds, a.iters)
        emit("")
        emit(f"SFNOBlock(width {C}, {nlat} x {nlon}, untruncated), bf16: sht -> mix -> isht -> fno_pointwise; "
             "mix=\"degree\": sfno_mix, mix=\"expand\": fno_mix on the bf16 expansion")
        emit("  " + _fmt("degree", t["degree"]) + " | " + _fmt("expand", t["expand"]) +
             f" | degree/expand {statistics.median(t['degree']) / statistics.median(t['expand']):.2f} | rel diff {diff:.1e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
