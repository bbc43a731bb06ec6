"""Spherical harmonic transforms: ``sht``, ``isht`` and the ``legendre`` op alone against the torch route --
``torch.fft.rfft`` / ``irfft`` (rocFFT) and an ``einsum`` on an fp32 Legendre table -- on the same inputs, hipGraph
timing, the two routes alternated round by round, median of the rounds.

  python bench/bench_sht.py [--rounds 7] [--dtype fp32] [--out profiles/sht_r10.txt]

Every shape is checked first: both routes against each other.  The ``legendre`` rows time the forward table
(``tri = 1``) on the spectrum the forward transform produces.

``--dtype bf16`` times the bf16 transforms instead, against the fp32 ones of the same op in the same process (the
same fields rounded to bf16), alternated the same way; the check is the bf16 result against the fp32 one.
profiles/sfno_bf16_r12.txt is this bench and bench_sfno_mix.py, the second appended to the first:

  python bench/bench_sht.py --dtype bf16 --out profiles/sfno_bf16_r12.txt
  python bench/bench_sfno_mix.py --dtype bf16 --out profiles/sfno_bf16_r12.txt --append
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrt_dft_plugins_amd as tdp  # noqa: E402
from bench.bench_fft import time_graph  # noqa: E402
from tensorrt_dft_plugins_amd.ops.sht import sht_tables  # noqa: E402

# (field [B, C, nlat, nlon], lmax = mmax or None for the untruncated default)
SHAPES = [((1, 20, 720, 1440), 64), ((1, 20, 720, 1440), 128), ((1, 64, 180, 360), None)]
GRID = "equiangular"


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of overwriting it")
    a = ap.parse_args(argv)
    tdp.load_plugins()
    ops = torch.ops.amd_dft
    dev = "cuda"
    if a.dtype == "bf16":
        return _main_bf16(a, ops, dev)
    lines = [f"Spherical harmonic transforms, fp32, {GRID} grid, hipGraph, median of {a.rounds} alternated rounds x "
             f"{a.iters} calls [min, max]; us per call; torch = torch.fft + einsum on an fp32 table",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for shape, trunc in SHAPES:
        torch.manual_seed(0)
        nlat, nlon = shape[-2:]
        lmax = trunc or nlat
        mmax = trunc or min(lmax, nlon // 2 + 1)
        t = sht_tables(nlat, nlon, lmax, mmax, GRID, dev)
        x = torch.randn(*shape, device=dev)
        c = tdp.sht(x, lmax, mmax, GRID)
        xf = ops.r2c(x, [3], 2.0 * math.pi / nlon, [mmax, 0], torch.float32)

        def sht_torch():
            f = torch.view_as_real(torch.fft.rfft(x, dim=-1, norm="forward")[..., :mmax]) * (2.0 * math.pi)
            return torch.einsum("mlk,bckmr->bclmr", t.fwd, f)

        def isht_torch():
            f = torch.einsum("mkl,bclmr->bckmr", t.inv, c)
            return torch.fft.irfft(torch.view_as_complex(f.contiguous()), n=nlon, dim=-1, norm="forward")

        rows = [("sht", lambda: tdp.sht(x, lmax, mmax, GRID), sht_torch),
                ("isht", lambda: tdp.isht(c, nlat, nlon, GRID), isht_torch),
                ("legendre", lambda: ops.legendre(xf, t.fwd, t.fwd_split, 1),
                 lambda: torch.einsum("mlk,bckmr->bclmr", t.fwd, xf))]
        emit(f"{list(shape)} lmax {lmax} mmax {mmax}   {ops.legendre_info(nlat, lmax, mmax, 2 * shape[0] * shape[1], 1)}")
        for name, new, old in rows:
            diff = _rel(new(), old())
            tn, to = [], []
            for _ in range(a.rounds):
                to.append(time_graph(old, a.iters))
                tn.append(time_graph(new, a.iters))
            mo, mn = statistics.median(to), statistics.median(tn)
            emit(f"  {name:<9} torch {mo:9.1f} us [{min(to):.1f}, {max(to):.1f}] | amd {mn:9.1f} us [{min(tn):.1f}, {max(tn):.1f}] | "
                 f"torch/amd {mo / mn:.2f} | rel diff {diff:.1e}")
        del x, c, xf
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write(("\n" if a.append else "") + "\n".join(lines) + "\n")


def _main_bf16(a, ops, dev):
    bf = torch.bfloat16
    lines = [f"Spherical harmonic transforms, bf16 against fp32 of the same op, {GRID} grid, hipGraph, median of "
             f"{a.rounds} alternated rounds x {a.iters} calls [min, max]; us per call",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for shape, trunc in SHAPES:
        torch.manual_seed(0)
        nlat, nlon = shape[-2:]
        lmax = trunc or nlat
        mmax = trunc or min(lmax, nlon // 2 + 1)
        t32 = sht_tables(nlat, nlon, lmax, mmax, GRID, dev)
        t16 = sht_tables(nlat, nlon, lmax, mmax, GRID, dev, bf)
        x16 = torch.randn(*shape, device=dev).to(bf)
        x32 = x16.float()
        c32 = tdp.sht(x32, lmax, mmax, GRID)
        c16 = c32.to(bf)
        xf32 = ops.r2c(x32, [3], 2.0 * math.pi / nlon, [mmax, 0], torch.float32)
        xf16 = xf32.to(bf)
        rows = [("sht", lambda: tdp.sht(x16, lmax, mmax, GRID), lambda: tdp.sht(x32, lmax, mmax, GRID)),
                ("isht", lambda: tdp.isht(c16, nlat, nlon, GRID), lambda: tdp.isht(c32, nlat, nlon, GRID)),
                ("legendre", lambda: ops.legendre(xf16, t16.fwd, t16.fwd_split, 1),
                 lambda: ops.legendre(xf32, t32.fwd, t32.fwd_split, 1))]
        cols = 2 * shape[0] * shape[1]
        emit(f"{list(shape)} lmax {lmax} mmax {mmax}   {ops.legendre_info(nlat, lmax, mmax, cols, 1, True)}")
        for name, new, old in rows:
            diff = _rel(new(), old())
            tn, to = [], []
            for _ in range(a.rounds):
                to.append(time_graph(old, a.iters))
                tn.append(time_graph(new, a.iters))
            mo, mn = statistics.median(to), statistics.median(tn)
            emit(f"  {name:<9} fp32 {mo:9.1f} us [{min(to):.1f}, {max(to):.1f}] | bf16 {mn:9.1f} us [{min(tn):.1f}, {max(tn):.1f}] | "
                 f"fp32/bf16 {mo / mn:.2f} | rel diff {diff:.1e}")
        del x16, x32, c16, c32, xf16, xf32
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write(("\n" if a.append else "") + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
