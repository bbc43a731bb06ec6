"""LayerNorm over the channels of NCHW fields: (a) the ``layer_norm_nchw`` op (csrc/spectral/layer_norm_nchw.hip)
against ``F.layer_norm`` on the permuted tensor -- the route a user has without it, permute + layer_norm + permute
back to a contiguous NCHW tensor; (b) ``fno_pointwise_ln``, the LayerNorm applied inside the MFMA 1x1 convolution,
against ``layer_norm_nchw`` followed by ``fno_pointwise``.  Both dtypes in one run.

  python bench/bench_layer_norm_nchw.py [--rounds 7] [--out profiles/layer_norm_nchw_r21.txt]

The hand kernels are timed as hipGraphs of ``--iters`` calls; the ATen route is timed EAGERLY (three launches, an
allocation per step).  Routes are alternated round by round, median of the rounds with [min, max].  GB/s counts one
read and one write of the tensor (what the resident route moves; the reread route reads its tile a second time, from
L2 where it fits); bench/membw.py gives the streaming rate to hold it against.  Every shape is checked first against
fp64.
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
from bench.bench_fft import time_eager, time_graph  # noqa: E402

SHAPES = [(1, 64, 180, 360), (1, 256, 180, 360), (1, 128, 45, 90)]
FUSED = [(64, 128), (256, 512)]  # Cin -> Cout at [1, Cin, 180, 360]
EPS = 1e-5


def _fmt(name, ts, nbytes=None):
    med = statistics.median(ts)
    s = f"{name} {med:9.1f} us [{min(ts):.1f}, {max(ts):.1f}]"
    return s if nbytes is None else s + f" {nbytes / med / 1e3:7.0f} GB/s"


def _timed(routes, rounds, iters):
    t = {name: [] for name, _, _ in routes}
    for _ in range(rounds):
        for name, fn, timer in routes:
            t[name].append(timer(fn, iters))
    return t


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    tdp.load_plugins()
    ops = torch.ops.amd_dft
    dev = "cuda"
    lines = [f"layer_norm_nchw / fno_pointwise_ln, affine, N(0, 1) inputs, median of {a.rounds} alternated rounds x "
             f"{a.iters} calls [min, max], us per call; hand kernels as hipGraphs, aten (permute + F.layer_norm + "
             f"permute back) EAGER; GB/s = (one read + one write of the tensor) / time",
             f"device: {torch.cuda.get_device_name(0)}"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    def ln_def(x, g, b):
        return F.layer_norm(x.movedim(1, -1), (x.shape[1],), g, b, EPS).movedim(-1, 1)

    with torch.no_grad():
        for dt, dname in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            emit("")
            emit(f"(a) layer_norm_nchw against aten, {dname}")
            for shape in SHAPES:
                torch.manual_seed(0)
                B, C = shape[:2]
                x = torch.randn(*shape, device=dev).to(dt)
                g, b = torch.randn(C, device=dev), torch.randn(C, device=dev)
                gt, bt = g.to(dt), b.to(dt)
                routes = [("aten", lambda: ln_def(x, gt, bt).contiguous(), time_eager),
                          ("layer_norm_nchw", lambda: ops.layer_norm_nchw(x, g, b, EPS), time_graph)]
                ref = ln_def(x.double(), g.double(), b.double())
                errs = [float((fn().double() - ref).abs().max()) for _, fn, _ in routes]
                del ref
                nbytes = 2 * x.numel() * x.element_size()
                emit(f"{list(shape)}  {nbytes / 2 ** 20:.1f} MiB read + written   "
                     f"{ops.layer_norm_nchw_info(B, C, x.numel() // (B * C), dt == torch.bfloat16)}")
                t = _timed(routes, a.rounds, a.iters)
                emit("  " + " | ".join(_fmt(n, t[n], nbytes) for n, _, _ in routes) +
                     f" | aten/layer_norm_nchw "
                     f"{statistics.median(t['aten']) / statistics.median(t['layer_norm_nchw']):.2f}"
                     f" | max abs err vs fp64: aten {errs[0]:.1e}, layer_norm_nchw {errs[1]:.1e}")
            emit("")
            emit(f"(b) fno_pointwise_ln against layer_norm_nchw + fno_pointwise, [1, Cin, 180, 360], GELU, {dname}")
            for cin, cout in FUSED:
                torch.manual_seed(0)
                x = torch.randn(1, cin, 180, 360, device=dev).to(dt)
                g, b = torch.randn(cin, device=dev), torch.randn(cin, device=dev)
                w, wb = torch.randn(cout, cin, device=dev) / cin ** 0.5, torch.randn(cout, device=dev)
                routes = [("ln + pointwise",
                           lambda: ops.fno_pointwise(None, ops.layer_norm_nchw(x, g, b, EPS), w, wb, True), time_graph),
                          ("fno_pointwise_ln", lambda: ops.fno_pointwise_ln(None, x, g, b, EPS, w, wb, True), time_graph),
                          ("pointwise alone", lambda: ops.fno_pointwise(None, x, w, wb, True), time_graph)]
                ref = F.gelu(torch.einsum("oi,bihw->bohw", w.double(), ln_def(x.double(), g.double(), b.double()))
                             + wb.double()[None, :, None, None])
                errs = [float((fn().double() - ref).norm() / ref.norm()) for _, fn, _ in routes[:2]]
                del ref
                t = _timed(routes, a.rounds, a.iters)
                emit(f"{cin} -> {cout}  " + " | ".join(_fmt(n, t[n]) for n, _, _ in routes) +
                     f" | unfused/fused "
                     f"{statistics.median(t['ln + pointwise']) / statistics.median(t['fno_pointwise_ln']):.2f}"
                     f" | rel-L2 vs fp64: unfused {errs[0]:.1e}, fused {errs[1]:.1e}")
                del x, routes
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
