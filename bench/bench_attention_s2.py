"""Neighbourhood attention on the sphere: the ``attention_s2`` op and the whole ``NeighborhoodAttentionS2`` module
against the route a user has without them -- the module's torch backend on the device, a masked softmax per output
latitude in eager torch -- on the same inputs.

  python bench/bench_attention_s2.py [--rounds 7] [--dtype both] [--out profiles/attention_s2_r18.txt]

The amd routes are timed as hipGraphs of ``--iters`` calls; the torch route launches several kernels per output
latitude and is timed eagerly between device synchronisations, one call per round.  Routes alternate round by round;
median of the rounds with [min, max].  Per shape the log also gives the neighbour pairs (scores that count) and how
many of them sit in the polar rows."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrt_dft_plugins_amd as tdp  # noqa: E402
from bench.bench_disco import _rel, time_eager_once  # noqa: E402
from bench.bench_fft import time_graph  # noqa: E402
from tensorrt_dft_plugins_amd.models import NeighborhoodAttentionS2  # noqa: E402
from tensorrt_dft_plugins_amd.ops.disco import default_cutoff  # noqa: E402

HEADS = 4
# (key / value [B, C, nlat, nlon], out grid, cutoff as a multiple of the default)
SHAPES = [((1, 64, 180, 360), (180, 360), 1), ((1, 64, 180, 360), (180, 360), 3), ((1, 64, 360, 720), (180, 360), 1)]


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
    lines = [f"Neighbourhood attention on the sphere, equiangular grids, {HEADS} heads, median of {a.rounds} alternated "
             f"rounds [min, max]; us per call; amd: hipGraph of {a.iters} calls; torch: the module's torch backend on "
             f"the device, eager, one call per round", f"device: {torch.cuda.get_device_name(0)}", ""]

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
        emit(f"  {name:<9} amd {mn:10.1f} us [{min(tn):.1f}, {max(tn):.1f}] | torch {mo:12.1f} us [{min(to):.1f}, "
             f"{max(to):.1f}] torch/amd {mo / mn:.1f} rel diff {d:.1e}")
        return mn

    for shape, outs, wide in SHAPES:
        torch.manual_seed(0)
        B, C, Hi, Wi = shape
        d = C // HEADS
        cut = wide * default_cutoff(1, outs[0])
        m = NeighborhoodAttentionS2(C, (Hi, Wi), outs, HEADS, theta_cutoff=cut).to(dev).eval()
        t = m.tables(dev)
        width = np.where(t.hw_host >= 0, np.minimum(2 * t.hw_host.astype(np.int64) + 1, Wi), 0)
        per_lat = width.sum(axis=1) * outs[1]
        pairs, cap = int(per_lat.sum()), max(1, outs[0] // 10)
        polar = int(per_lat[:cap].sum() + per_lat[-cap:].sum())
        emit(f"{list(shape)} -> {list(outs)} cutoff {wide} x default = {cut:.4f}: {pairs} neighbour pairs per (b, head), "
             f"polar rows (first and last {cap} latitudes) {100.0 * polar / pairs:.1f} %; input rows per output "
             f"latitude max {int((t.hw_host >= 0).sum(axis=1).max())}; hw at the equator "
             f"{int(t.hw_host[outs[0] // 2].max())}")
        q32 = torch.randn(B, C, *outs, device=dev).to(bf).float()
        k32 = torch.randn(*shape, device=dev).to(bf).float()
        v32 = torch.randn(*shape, device=dev).to(bf).float()
        for dt in ([torch.float32, bf] if a.dtype == "both" else [torch.float32 if a.dtype == "fp32" else bf]):
            q, k, v = q32.to(dt), k32.to(dt), v32.to(dt)
            name = "fp32" if dt == torch.float32 else "bf16"
            emit(f" {name}   {ops.attention_s2_info(B, HEADS, d, Hi, Wi, outs[0], outs[1], dt == bf)}")
            with torch.no_grad():
                ta = race("attention", lambda: tdp.attention_s2(q, k, v, t, m.scale, HEADS),
                          lambda: m.attend_torch(q.float(), k.float(), v.float()).to(dt))

                def amd_module():
                    m.backend = "amd"
                    return m(q, k)

                def torch_module():
                    m.backend = "torch"
                    return m(q, k)

                race("module", amd_module, torch_module)
                m.backend = "amd"
            flops = 4.0 * pairs * d * B * HEADS  # q.k and p.v of the pairs that count
            emit(f"  attention: {flops / ta / 1e6:.2f} TFLOP/s over the neighbour pairs alone (2 x 2 d per pair); "
                 f"{pairs * B * HEADS / ta / 1e3:.2f} G pairs/s")
        del m
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
