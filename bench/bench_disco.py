"""Discrete-continuous convolutions on the sphere: the ``disco`` op and the whole ``DiscreteContinuousConvS2``
module against the route a user has without them -- the module's torch backend on the device, a sparse matrix
applied at every output longitude in eager torch -- on the same inputs.

  python bench/bench_disco.py [--rounds 7] [--dtype both] [--out profiles/disco_r16.txt]

The amd routes are timed as hipGraphs of ``--iters`` calls; the torch route launches nlon_out sparse products per
call and is timed eagerly between device synchronisations, one call per round.  Routes alternate round by round;
median of the rounds with [min, max].  Per shape the log also gives the nnz split between polar and equatorial rows,
the bytes the op has to move (x once, y once) and what ``bench/membw.py`` copies at that size in the same run."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrt_dft_plugins_amd as tdp  # noqa: E402
from bench import membw  # noqa: E402
from bench.bench_fft import time_graph  # noqa: E402
from tensorrt_dft_plugins_amd.models import DiscreteContinuousConvS2  # noqa: E402

# (x [B, C, nlat, nlon], out grid, kernel_shape)
SHAPES = [((1, 20, 720, 1440), (360, 720), 3), ((1, 64, 180, 360), (180, 360), (3, 4))]


def time_eager_once(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dtype", choices=["fp32", "bf16", "both"], default="both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    tdp.load_plugins()
    ops = torch.ops.amd_dft
    dev, bf = "cuda", torch.bfloat16
    lines = [f"DISCO convolutions, equiangular grids, median of {a.rounds} alternated rounds [min, max]; us per call; "
             f"amd: hipGraph of {a.iters} calls; torch: the module's torch backend on the device, eager, one call per "
             f"round", f"device: {torch.cuda.get_device_name(0)}", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    def race(name, new, old):
        d = _rel(new(), old())
        tn, to = [], []
        for _ in range(a.rounds):
            to.append(time_eager_once(old))
            tn.append(time_graph(new, a.iters))
        mn, mo = statistics.median(tn), statistics.median(to)
        emit(f"  {name:<7} amd {mn:10.1f} us [{min(tn):.1f}, {max(tn):.1f}] | torch {mo:12.1f} us [{min(to):.1f}, "
             f"{max(to):.1f}] torch/amd {mo / mn:.1f} rel diff {d:.1e}")
        return mn

    for shape, outs, ks in SHAPES:
        torch.manual_seed(0)
        B, C, Hi, Wi = shape
        m = DiscreteContinuousConvS2(C, C, (Hi, Wi), outs, ks).to(dev).eval()
        t = m.tables(dev)
        rows = np.diff(t.row_ptr_host.astype(np.int64)).reshape(t.K, outs[0])
        per_lat = rows.sum(axis=0)
        cap = max(1, outs[0] // 10)
        polar = int(per_lat[:cap].sum() + per_lat[-cap:].sum())
        emit(f"{list(shape)} -> {list(outs)} kernel_shape {ks} K {t.K} nnz {t.nnz}: polar rows (first and last "
             f"{cap} latitudes) {polar} = {100.0 * polar / t.nnz:.1f} %, the other {outs[0] - 2 * cap} latitudes "
             f"{t.nnz - polar}; entries per (p, k') row max {int(rows.max())} median {int(np.median(rows))}; "
             f"gathered products per plane {int(per_lat.sum()) * outs[1]}")
        x32 = torch.randn(*shape, device=dev).to(bf).float()
        for dt in ([torch.float32, bf] if a.dtype == "both" else [torch.float32 if a.dtype == "fp32" else bf]):
            x = x32.to(dt)
            name = "fp32" if dt == torch.float32 else "bf16"
            emit(f" {name}   {ops.disco_info(B * C, Hi, Wi, t.K, outs[0], outs[1], t.nnz, dt == bf)}")
            with torch.no_grad():
                gather_ref = (lambda: m.gather_torch(x.float()).to(dt))
                td = race("disco", lambda: tdp.disco(x, t), gather_ref)

                def amd_module():
                    m.backend = "amd"
                    return m(x)

                def torch_module():
                    m.backend = "torch"
                    return m(x)

                race("module", amd_module, torch_module)
                m.backend = "amd"
            nbytes = (x.numel() + B * C * t.K * outs[0] * outs[1]) * x.element_size()
            (r,) = membw.main(["--mb", f"{nbytes / 1e6:.1f}", "--iters", str(a.iters)])
            products = int(per_lat.sum()) * outs[1] * B * C
            emit(f"  disco moves {nbytes / 1e6:.1f} MB (x once, y once): {nbytes / td / 1e6:.3f} TB/s; a copy of a "
                 f"buffer that size runs at {r['copy_TBps(r+w)']:.2f} TB/s (r+w) in this run; {products / td / 1e6:.2f} T "
                 f"gathered products/s")
        del m, x32
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
