"""Vector spherical harmonic transforms: the fused ``legendre_vec`` kernel against the two routes it replaces, and
``vsht`` / ``ivsht`` against the torch backend, on the same inputs; hipGraph timing, the routes alternated round by
round, median of the rounds.

  python bench/bench_vsht.py [--rounds 7] [--dtype both] [--out profiles/vsht_r15.txt]

``legendre_vec`` rows (the forward tables, ``tri = 1``, on the spectrum the forward transform produces):
  (a) "4xlegendre": the composition out of existing ops -- four ``legendre`` calls on the same (pre-split) tables, on
      contiguous copies of the two components made outside the timed region, plus the combine (fp32: two complex
      ``torch.add(.., alpha=-/+i)`` into the result; bf16, where complex does not exist: the rotations as
      ``stack`` / ``neg`` and two adds);
  (b) "einsum": ``torch.einsum`` of both fp32 tables with the fp32 spectrum plus the same complex combine.
``vsht`` / ``ivsht`` rows: against the torch backend's route in fp32 (``torch.fft`` + einsum on the fp32 tables + the
complex combine).  Every row is checked first: the routes against each other."""
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
from tensorrt_dft_plugins_amd.ops.sht import vsht_tables  # noqa: E402

# (field [B, C, 2, nlat, nlon], lmax = mmax or None for the untruncated default)
SHAPES = [((1, 10, 2, 720, 1440), 64), ((1, 10, 2, 720, 1440), 128), ((1, 32, 2, 180, 360), None)]
GRID = "equiangular"


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _combine_complex(a, b, out):
    """out[:, :, 0] = a0 - i b1, out[:, :, 1] = a1 + i b0 on [B, C, 2, R, M, 2] fp32 tensors: two element-wise ops."""
    ac, bc, oc = (torch.view_as_complex(t) for t in (a, b, out))
    torch.add(ac[:, :, 0], bc[:, :, 1], alpha=-1j, out=oc[:, :, 0])
    torch.add(ac[:, :, 1], bc[:, :, 0], alpha=1j, out=oc[:, :, 1])
    return out


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
    lines = [f"Vector spherical harmonic transforms, {GRID} grid, hipGraph, median of {a.rounds} alternated rounds x "
             f"{a.iters} calls [min, max]; us per call",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    def race(name, new, others):
        """``new`` against each (label, fn) of ``others``, all alternated in every round."""
        diffs = [_rel(new(), fn()) for _, fn in others]
        tn, to = [], [[] for _ in others]
        for _ in range(a.rounds):
            for ts, (_, fn) in zip(to, others):
                ts.append(time_graph(fn, a.iters))
            tn.append(time_graph(new, a.iters))
        mn = statistics.median(tn)
        s = f"  {name:<13} amd {mn:9.1f} us [{min(tn):.1f}, {max(tn):.1f}]"
        for ts, (label, _), d in zip(to, others, diffs):
            mo = statistics.median(ts)
            s += f" | {label} {mo:9.1f} us [{min(ts):.1f}, {max(ts):.1f}] {label}/amd {mo / mn:.2f} rel diff {d:.1e}"
        emit(s)

    for shape, trunc in SHAPES:
        torch.manual_seed(0)
        nlat, nlon = shape[-2:]
        lmax = trunc or nlat
        mmax = trunc or min(lmax, nlon // 2 + 1)
        cols = 4 * shape[0] * shape[1]
        t32 = vsht_tables(nlat, nlon, lmax, mmax, GRID, dev)
        x32 = torch.randn(*shape, device=dev).to(bf).float()
        c32 = tdp.vsht(x32, lmax, mmax, GRID)
        xf32 = ops.r2c(x32, [4], 2.0 * math.pi / nlon, [mmax, 0], torch.float32)  # [B, C, 2, nlat, mmax, 2]
        out32 = torch.empty_like(c32)

        def einsum32():
            ea = torch.einsum("mlk,bcvkmr->bcvlmr", t32.fwd_a, xf32)
            eb = torch.einsum("mlk,bcvkmr->bcvlmr", t32.fwd_b, xf32)
            return _combine_complex(ea, eb, out32)

        def vsht_torch():
            f = torch.view_as_real(torch.fft.rfft(x32, dim=-1, norm="forward")[..., :mmax]) * (2.0 * math.pi)
            ea = torch.einsum("mlk,bcvkmr->bcvlmr", t32.fwd_a, f)
            eb = torch.einsum("mlk,bcvkmr->bcvlmr", t32.fwd_b, f)
            return _combine_complex(ea, eb, out32)

        def ivsht_torch():
            ea = torch.einsum("mkl,bcvlmr->bcvkmr", t32.inv_a, c32)
            eb = torch.einsum("mkl,bcvlmr->bcvkmr", t32.inv_b, c32)
            f = _combine_complex(ea, eb, torch.empty_like(ea))
            return torch.fft.irfft(torch.view_as_complex(f), n=nlon, dim=-1, norm="forward")

        for dt in ([torch.float32, bf] if a.dtype == "both" else [torch.float32 if a.dtype == "fp32" else bf]):
            t = t32 if dt == torch.float32 else vsht_tables(nlat, nlon, lmax, mmax, GRID, dev, bf)
            x, c, xf = x32.to(dt), c32.to(dt), xf32.to(dt)
            x0, x1 = xf[:, :, 0].contiguous(), xf[:, :, 1].contiguous()
            out = torch.empty_like(c)

            def four():
                a0 = ops.legendre(x0, t.fwd_a, t.fwd_a_split, 1)
                a1 = ops.legendre(x1, t.fwd_a, t.fwd_a_split, 1)
                b0 = ops.legendre(x0, t.fwd_b, t.fwd_b_split, 1)
                b1 = ops.legendre(x1, t.fwd_b, t.fwd_b_split, 1)
                if dt == torch.float32:
                    torch.add(torch.view_as_complex(a0), torch.view_as_complex(b1), alpha=-1j,
                              out=torch.view_as_complex(out)[:, :, 0])
                    torch.add(torch.view_as_complex(a1), torch.view_as_complex(b0), alpha=1j,
                              out=torch.view_as_complex(out)[:, :, 1])
                else:
                    torch.add(a0, torch.stack([b1[..., 1], -b1[..., 0]], -1), out=out[:, :, 0])
                    torch.add(a1, torch.stack([-b0[..., 1], b0[..., 0]], -1), out=out[:, :, 1])
                return out

            name = "fp32" if dt == torch.float32 else "bf16"
            emit(f"{list(shape)} lmax {lmax} mmax {mmax} {name}   "
                 f"{ops.legendre_vec_info(nlat, lmax, mmax, cols, 1, dt == bf)}")
            race("legendre_vec", lambda: ops.legendre_vec(xf, t.fwd_a, t.fwd_b, t.fwd_a_split, t.fwd_b_split, 1),
                 [("4xlegendre", four), ("einsum", einsum32)])
            race("vsht", lambda: tdp.vsht(x, lmax, mmax, GRID), [("torch", vsht_torch)])
            race("ivsht", lambda: tdp.ivsht(c, nlat, nlon, GRID), [("torch", ivsht_torch)])
            del x, c, xf, x0, x1, out
        del x32, c32, xf32, out32
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
