"""The transposed (upsampling) DISCO convolution: the ``disco_t`` op and the whole
``DiscreteContinuousConvTransposeS2`` module against the route a user has without them -- the module's torch backend
on the device, a sparse matrix applied once per input longitude in eager torch -- on the same inputs, and against
the forward ``disco`` op on the mirrored shape (fine grid -> coarse grid, the same basis: about the same nnz and the
same bytes, read and written the other way round) as a yardstick.

  python bench/bench_disco_t.py [--rounds 7] [--dtype both] [--out profiles/disco_t_r17.txt]

The amd routes are timed as hipGraphs of ``--iters`` calls; the torch route launches nlon_in sparse products per call
and is timed eagerly between device synchronisations, one call per round.  Routes alternate round by round; median
of the rounds with [min, max]."""
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
from tensorrt_dft_plugins_amd.models import DiscreteContinuousConvS2, DiscreteContinuousConvTransposeS2  # noqa: E402

# (x [B, C, nlat_in, nlon_in], out grid, kernel_shape)
SHAPES = [((1, 20, 360, 720), (720, 1440), 3), ((1, 64, 180, 360), (180, 360), (3, 4))]


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
    lines = [f"Transposed DISCO convolutions, equiangular grids, median of {a.rounds} alternated rounds [min, max]; us "
             f"per call; amd: hipGraph of {a.iters} calls; torch: the module's torch backend on the device, eager, one "
             f"call per round", f"device: {torch.cuda.get_device_name(0)}", ""]

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
        m = DiscreteContinuousConvTransposeS2(C, C, (Hi, Wi), outs, ks).to(dev).eval()
        with torch.no_grad():
            m.bias.normal_()
        t = m.tables(dev)
        fwd = DiscreteContinuousConvS2(C, C, outs, (Hi, Wi), ks).tables(dev)
        rows = np.diff(t.row_ptr_host.astype(np.int64)).reshape(outs[0], t.s)
        per_lat = rows.sum(axis=1)
        kin = t.idx.cpu().numpy().astype(np.int64) // (t.K * Wi)
        rp = t.row_ptr_host.astype(np.int64)
        bands = [int(kin[rp[k * t.s]:rp[(k + 1) * t.s]].max() - kin[rp[k * t.s]:rp[(k + 1) * t.s]].min()) + 1
                 for k in range(outs[0])]
        emit(f"{list(shape)} -> {list(outs)} kernel_shape {ks} K {t.K} s {t.s} nnz {t.nnz} (forward table of the "
             f"mirrored shape: {fwd.nnz}); entries per (k, rho) row max {int(rows.max())} median "
             f"{int(np.median(rows))}; band of input latitudes per output latitude max {max(bands)} median "
             f"{int(np.median(bands))}; gathered products per plane {int(per_lat.sum()) * Wi}")
        z32 = torch.randn(B, C, t.K, Hi, Wi, device=dev).to(bf).float()
        x32 = torch.randn(*shape, device=dev).to(bf).float()
        xf32 = torch.randn(B, C, *outs, device=dev).to(bf).float()
        bias = m.bias.detach().float()
        for dt in ([torch.float32, bf] if a.dtype == "both" else [torch.float32 if a.dtype == "fp32" else bf]):
            z, x, xf = z32.to(dt), x32.to(dt), xf32.to(dt)
            name = "fp32" if dt == torch.float32 else "bf16"
            emit(f" {name}   {ops.disco_t_info(B * C, Hi, Wi, t.K, outs[0], outs[1], t.nnz, dt == bf)}")
            with torch.no_grad():
                gather_ref = (lambda: (m.gather_torch(z.float()) + bias[None, :, None, None]).to(dt))
                td = race("disco_t", lambda: tdp.disco_transpose(z, t, bias), gather_ref)

                def amd_module():
                    m.backend = "amd"
                    return m(x)

                def torch_module():
                    m.backend = "torch"
                    return m(x)

                race("module", amd_module, torch_module)
                m.backend = "amd"
                tf = [time_graph(lambda: tdp.disco(xf, fwd), a.iters) for _ in range(a.rounds)]
            mf = statistics.median(tf)
            nbytes = (z.numel() + B * C * outs[0] * outs[1]) * z.element_size()
            products = int(per_lat.sum()) * Wi * B * C
            emit(f"  forward disco on the mirrored shape {list(xf.shape)} -> {[Hi, Wi]}: {mf:.1f} us [{min(tf):.1f}, "
                 f"{max(tf):.1f}]; disco_t / disco {td / mf:.2f}")
            emit(f"  disco_t moves {nbytes / 1e6:.1f} MB (z once, y once): {nbytes / td / 1e6:.3f} TB/s; "
                 f"{products / td / 1e6:.2f} T gathered products/s")
        del m, z32, x32, xf32
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
