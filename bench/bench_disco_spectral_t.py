"""The longitude-Fourier route of the transposed DISCO convolution against the gather route, same inputs, same
process: ``disco_spectral_transpose`` whole (``r2c``, the ``disco_spectral_t`` op, ``c2r``) and the op alone against
``disco_t``, on the two shapes of ``bench/bench_disco_t.py``, fp32 and bf16, with bias.

  python bench/bench_disco_spectral_t.py [--rounds 7] [--iters 10] [--out profiles/disco_spectral_t_r20.txt]

Every route is timed as a hipGraph of ``--iters`` calls; the routes alternate round by round; median of the rounds
with [min, max]."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrt_dft_plugins_amd as tdp  # noqa: E402
from bench.bench_disco_t import SHAPES  # noqa: E402
from bench.bench_fft import time_graph  # noqa: E402
from tensorrt_dft_plugins_amd.ops import disco as D  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    tdp.load_plugins()
    ops = torch.ops.amd_dft
    dev, bf = "cuda", torch.bfloat16
    lines = [f"transposed DISCO, longitude-Fourier route against the gather route, equiangular grids; us per call, "
             f"hipGraphs of {a.iters} calls, median of {a.rounds} alternated rounds [min, max]",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for shape, outs, ks in SHAPES:
        torch.manual_seed(0)
        B, C, Hi, Wi = shape
        tg = D.disco_transpose_table_holder((Hi, Wi), outs, ks, device=dev)
        ts = D.disco_spectral_transpose_table_holder((Hi, Wi), outs, ks, device=dev)
        emit(f"z {[B, C, ts.K, Hi, Wi]} -> {list(outs)} kernel_shape {ks} K {ts.K}: gather nnz {tg.nnz}; spectral U {ts.U} "
             f"KD {ts.KD} s {ts.s} Mo {ts.Mo} table {ts.table_bytes / 1e6:.1f} MB (bf16 plane {ts.table_bytes / 2e6:.1f} MB)")
        z32 = torch.randn(B, C, ts.K, Hi, Wi, device=dev)  # plain fp32 values: the lo plane of the staged spectrum is live
        bias = torch.randn(C, device=dev)
        for dt in (torch.float32, bf):
            z = z32.to(dt)
            name = "fp32" if dt == torch.float32 else "bf16"
            table = ts.table_bf16 if dt == bf else ts.table
            emit(f" {name}   {ops.disco_spectral_t_info(B * C, Hi, Wi, ts.K, outs[0], outs[1], ts.U, dt == bf)}")
            with torch.no_grad():
                zh = ops.r2c(z, [4], 1.0, [], dt)
                routes = {
                    "disco_t (gather)": lambda: tdp.disco_transpose(z, tg, bias),
                    "disco_spectral_transpose (r2c + op + c2r)": lambda: tdp.disco_spectral_transpose(z, ts, bias),
                    "disco_spectral_t op alone": lambda: ops.disco_spectral_t(zh, table, ts.lo, ts.K, ts.U, outs[0], Wi,
                                                                              outs[1], bias),
                }
                ref = routes["disco_t (gather)"]().double()
                d = float((routes["disco_spectral_transpose (r2c + op + c2r)"]().double() - ref).norm() / ref.norm())
                times = {k: [] for k in routes}
                for _ in range(a.rounds):
                    for k, fn in routes.items():
                        times[k].append(time_graph(fn, a.iters))
            base = statistics.median(times["disco_t (gather)"])
            for k, t in times.items():
                med = statistics.median(t)
                emit(f"  {k:<42} {med:9.1f} us [{min(t):.1f}, {max(t):.1f}]  gather / this {base / med:5.2f}")
            emit(f"  spectral against gather, whole result: rel diff {d:.1e}")
        del z32
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
