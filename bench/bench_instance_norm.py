"""Instance normalisation: the ``instance_norm`` op (csrc/spectral/instance_norm.hip) against
``torch.nn.functional.instance_norm`` on the device -- the route a user has without it -- on the same inputs, hipGraph
timing, the two alternated round by round, median of the rounds.  Last line: a whole ``SFNONet`` forward, the amd
backend (hipGraph) against the torch backend (eager).

  python bench/bench_instance_norm.py [--rounds 7] [--dtype fp32] [--out profiles/instance_norm_r13.txt] [--append]

Effective GB/s counts one read and one write of the tensor (the resident route's traffic; the split route moves the
input twice, so at the same HBM rate it shows two thirds of the figure).  bench/membw.py gives the streaming rate to
hold it against.  Every shape is checked first: the op against ATen in fp64.
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
from tensorrt_dft_plugins_amd.models import SFNOConfig, SFNONet  # noqa: E402

SHAPES = [(1, 64, 180, 360), (1, 256, 360, 720), (1, 20, 720, 1440)]
NET = dict(img_size=(180, 360), in_chans=20, out_chans=20, embed_dim=64, depth=4)  # untruncated
EPS = 1e-6


def _timed(routes, rounds, iters):
    t = {name: [] for name, _ in routes}
    for _ in range(rounds):
        for name, fn in routes:
            t[name].append(time_graph(fn, iters))
    return t


def _fmt(name, ts, nbytes=None):
    med = statistics.median(ts)
    s = f"{name} {med:9.1f} us [{min(ts):.1f}, {max(ts):.1f}]"
    return s if nbytes is None else s + f" {nbytes / med / 1e3:7.0f} GB/s"


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
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    lines = [f"instance_norm, {a.dtype}, affine, N(0, 1) inputs, hipGraph, median of {a.rounds} alternated rounds x "
             f"{a.iters} calls [min, max]; us per call; GB/s = (one read + one write of the tensor) / time; "
             f"aten = torch.nn.functional.instance_norm", f"device: {torch.cuda.get_device_name(0)}", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    with torch.no_grad():
        for shape in SHAPES:
            torch.manual_seed(0)
            B, C = shape[:2]
            x = torch.randn(*shape, device=dev).to(dt)
            w, b = torch.randn(C, device=dev), torch.randn(C, device=dev)
            wt, bt = w.to(dt), b.to(dt)  # ATen wants the affine parameters in x's dtype
            routes = [("aten", lambda: F.instance_norm(x, weight=wt, bias=bt, eps=EPS)),
                      ("instance_norm", lambda: ops.instance_norm(x, w, b, EPS))]
            ref = F.instance_norm(x.double(), weight=w.double(), bias=b.double(), eps=EPS)
            errs = [float((fn().double() - ref).abs().max()) for _, fn in routes]
            del ref
            nbytes = 2 * x.numel() * x.element_size()
            emit(f"{list(shape)}  {nbytes / 2 ** 20:.0f} MiB read + written   "
                 f"{ops.instance_norm_info(B * C, x.numel() // (B * C), a.dtype == 'bf16')}")
            t = _timed(routes, a.rounds, a.iters)
            emit("  " + " | ".join(_fmt(name, t[name], nbytes) for name, _ in routes) +
                 f" | aten/instance_norm {statistics.median(t['aten']) / statistics.median(t['instance_norm']):.2f}"
                 f" | max abs err vs fp64: aten {errs[0]:.1e}, instance_norm {errs[1]:.1e}")
            del x, routes
            torch.cuda.empty_cache()

        torch.manual_seed(0)
        net = SFNONet(SFNOConfig(**NET)).to(dev).eval()
        x = torch.randn(1, NET["in_chans"], *NET["img_size"], device=dev).to(dt)
        ref = net.set_backend("torch")(x.double())
        routes = [("amd", lambda: net.set_backend("amd")(x))]
        if a.dtype == "fp32":  # the torch backend has no bf16 route (torch.fft takes none)
            routes.insert(0, ("torch", lambda: net.set_backend("torch")(x)))
        diff = float((net.set_backend("amd")(x).double() - ref).norm() / ref.norm())
        # the torch backend is timed eagerly (time_eager): torch.fft plans are not all capturable; its forward is
        # long enough for launch overhead not to matter
        iters = max(a.iters // 2, 2)
        t = {name: [] for name, _ in routes}
        for _ in range(a.rounds):
            for name, fn in routes:
                t[name].append((time_graph if name == "amd" else time_eager)(fn, iters))
        emit("")
        emit(f"SFNONet(embed {NET['embed_dim']}, depth {NET['depth']}, {NET['img_size'][0]} x {NET['img_size'][1]}, "
             f"untruncated, batch 1), whole forward")
        row = "  " + " | ".join(_fmt(name, t[name]) for name, _ in routes)
        if "torch" in t:
            row += f" | torch/amd {statistics.median(t['torch']) / statistics.median(t['amd']):.2f}"
        emit(row + f" | amd rel-L2 against the fp64 torch backend {diff:.1e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write(("\n" if a.append else "") + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
