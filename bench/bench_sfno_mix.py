"""SFNO per-degree channel mixing: the ``sfno_mix`` op against the routes it replaces -- complex
``torch.einsum("bilm,iol->bolm")`` (what the layer ran above the expansion bound) and, where the expansion fits under
the bound, ``fno_mix`` on the weights expanded over every order -- on the same inputs, hipGraph timing, the routes
alternated round by round, median of the rounds.  Last line: a whole ``SFNOBlock`` with ``mix="degree"``.

  python bench/bench_sfno_mix.py [--rounds 7] [--dtype fp32] [--out profiles/sfno_mix_r11.txt]

Every shape is checked first: the routes against each other.  The spectra are ``sht`` of random fields (zero where
l < m), mixed with ``tri = 1`` as the layers do.

``--dtype bf16`` times the bf16 ``sfno_mix`` and the bf16 ``SFNOBlock`` instead, against the fp32 ones in the same
process (the same spectra, fields and weights rounded to bf16), alternated the same way; the check is the bf16 result
against the fp32 one.  The last line is a layer below the expansion bound with ``mix="auto"``: there the fp32 layer
mixes with ``fno_mix`` on expanded weights and the bf16 layer with ``sfno_mix`` (``fno_mix`` has no bf16 kernel), the
one pairing where the bf16 mix op is the slower of the two on its own.  (``--append``: add to ``--out``; see
bench_sht.py for the two commands behind profiles/sfno_bf16_r12.txt.)
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrt_dft_plugins_amd as tdp  # noqa: E402
from bench.bench_fft import time_graph  # noqa: E402
from tensorrt_dft_plugins_amd.models import sfno  # noqa: E402
from tensorrt_dft_plugins_amd.ops import spectral as SP  # noqa: E402

# spectra [B, C, L, M] (C = Cin = Cout), from fields [B, C, nlat = L, nlon = 2 M]
SHAPES = [(1, 20, 64, 64), (4, 64, 128, 128), (1, 64, 180, 180), (1, 256, 180, 180)]
BLOCK = (1, 64, 180, 360)  # the SFNOBlock line: width 64 on 180 x 360, untruncated
SMALL_BLOCK = (1, 20, 64, 128)  # --dtype bf16: a layer whose expansion (12 MiB) is below the bound
GRID = "equiangular"


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _timed(routes, rounds, iters):
    """{name: [us per round]} with the routes alternated round by round."""
    t = {name: [] for name, _ in routes}
    for _ in range(rounds):
        for name, fn in routes:
            t[name].append(time_graph(fn, iters))
    return t


def _fmt(name, ts):
    return f"{name} {statistics.median(ts):9.1f} us [{min(ts):.1f}, {max(ts):.1f}]"


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
    lines = [f"SFNO per-degree mixing, fp32, spectra of random fields ({GRID} grid), tri = 1, hipGraph, median of "
             f"{a.rounds} alternated rounds x {a.iters} calls [min, max]; us per call; einsum = complex64 torch.einsum, "
             f"expanded = fno_mix on weights expanded over m (where they fit under {sfno.EXPAND_LIMIT_BYTES >> 20} MiB)",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    with torch.no_grad():
        for B, C, L, M in SHAPES:
            torch.manual_seed(0)
            c = tdp.sht(torch.randn(B, C, L, 2 * M, device=dev), L, M, GRID)  # [B, C, L, M, 2]
            w = torch.rand(C, C, L, 2, device=dev) / (C * C)
            ws = SP.sfno_mix_split(w)
            cc, wc = torch.view_as_complex(c), torch.view_as_complex(w)
            routes = [("einsum", lambda: torch.einsum("bilm,iol->bolm", cc, wc)),
                      ("sfno_mix", lambda: ops.sfno_mix(c, w, ws, 1))]
            ref = torch.view_as_real(routes[0][1]())
            diffs = [f"sfno_mix vs einsum {_rel(routes[1][1](), ref):.1e}"]
            expanded = C * C * L * M * 8
            if expanded <= sfno.EXPAND_LIMIT_BYTES:
                we = w[:, :, :, None, :].expand(-1, -1, -1, M, -1).reshape(C, C, L * M, 2).contiguous()
                cf = c.reshape(B, C, L * M, 2)
                routes.append(("expanded", lambda: ops.fno_mix(cf, we, 0)))
                diffs.append(f"expanded vs einsum {_rel(routes[2][1]().reshape(ref.shape), ref):.1e}")
            emit(f"[{B}, {C}, {L}, {M}]  expansion {expanded / 2 ** 20:.0f} MiB, table {ws.numel() * 2 / 2 ** 20:.1f} MiB   "
                 f"{ops.sfno_mix_info(B, C, C, L, M, 1)}")
            t = _timed(routes, a.rounds, a.iters)
            mn = statistics.median(t["sfno_mix"])
            row = "  " + " | ".join(_fmt(name, t[name]) for name, _ in routes)
            row += f" | einsum/sfno_mix {statistics.median(t['einsum']) / mn:.2f}"
            if "expanded" in t:
                row += f" | expanded/sfno_mix {statistics.median(t['expanded']) / mn:.2f}"
            emit(row + " | rel diff " + ", ".join(diffs))
            del c, w, ws, cc, wc, ref, routes
            torch.cuda.empty_cache()

        B, C, nlat, nlon = BLOCK
        torch.manual_seed(0)
        x = torch.randn(B, C, nlat, nlon, device=dev)
        blk = sfno.SFNOBlock(C, nlat, nlon, grid=GRID, backend="amd", mix="degree").to(dev).eval()
        diff = _rel(blk(x), blk.set_backend("torch")(x))
        blk.set_backend("amd")
        t = _timed([("amd", lambda: blk(x))], a.rounds, a.iters)
        emit("")
        emit(f"SFNOBlock(width {C}, {nlat} x {nlon}, untruncated, mix=\"degree\"): sht -> sfno_mix -> isht -> fno_pointwise")
        emit("  " + _fmt("amd", t["amd"]) + f" | rel diff against the torch backend {diff:.1e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write(("\n" if a.append else "") + "\n".join(lines) + "\n")


def _main_bf16(a, ops, dev):
    bf = torch.bfloat16
    lines = [f"SFNO per-degree mixing, bf16 against fp32 of the same op, spectra of random fields ({GRID} grid), tri = 1, "
             f"hipGraph, median of {a.rounds} alternated rounds x {a.iters} calls [min, max]; us per call",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    with torch.no_grad():
        for B, C, L, M in SHAPES:
            torch.manual_seed(0)
            c16 = tdp.sht(torch.randn(B, C, L, 2 * M, device=dev), L, M, GRID).to(bf)  # [B, C, L, M, 2]
            w16 = (torch.rand(C, C, L, 2, device=dev) / (C * C)).to(bf)
            c32, w32 = c16.float(), w16.float()
            ws16, ws32 = SP.sfno_mix_split(w16), SP.sfno_mix_split(w32)
            routes = [("fp32", lambda: ops.sfno_mix(c32, w32, ws32, 1)), ("bf16", lambda: ops.sfno_mix(c16, w16, ws16, 1))]
            diff = _rel(routes[1][1](), routes[0][1]())
            emit(f"[{B}, {C}, {L}, {M}]  table {ws16.numel() * 2 / 2 ** 20:.1f} MiB (fp32: {ws32.numel() * 2 / 2 ** 20:.1f})   "
                 f"{ops.sfno_mix_info(B, C, C, L, M, 1, True)}")
            t = _timed(routes, a.rounds, a.iters)
            emit("  " + " | ".join(_fmt(name, t[name]) for name, _ in routes) +
                 f" | fp32/bf16 {statistics.median(t['fp32']) / statistics.median(t['bf16']):.2f} | rel diff {diff:.1e}")
            del c16, c32, w16, w32, ws16, ws32, routes
            torch.cuda.empty_cache()

        # width 64 untruncated: sfno_mix in both dtypes under either mix value (1 GiB of expansion); the small layer
        # under "auto": fp32 on fno_mix with expanded weights, bf16 on sfno_mix
        for (B, C, nlat, nlon), mix in ((BLOCK, "degree"), (SMALL_BLOCK, "auto")):
            torch.manual_seed(0)
            x16 = torch.randn(B, C, nlat, nlon, device=dev).to(bf)
            x32 = x16.float()
            blk = sfno.SFNOBlock(C, nlat, nlon, grid=GRID, backend="amd", mix=mix).to(dev).eval()
            diff = _rel(blk(x16), blk(x32))
            t = _timed([("fp32", lambda: blk(x32)), ("bf16", lambda: blk(x16))], a.rounds, a.iters)
            emit("")
            route = "fno_mix (expanded)" if blk.spectral.expanded_bytes() <= sfno.EXPAND_LIMIT_BYTES and mix == "auto" \
                else "sfno_mix"
            emit(f"SFNOBlock(width {C}, {nlat} x {nlon}, untruncated, mix=\"{mix}\"): sht -> mix -> isht -> fno_pointwise; "
                 f"mix op: fp32 {route}, bf16 sfno_mix")
            emit("  " + _fmt("fp32", t["fp32"]) + " | " + _fmt("bf16", t["bf16"]) +
                 f" | fp32/bf16 {statistics.median(t['fp32']) / statistics.median(t['bf16']):.2f} | rel diff {diff:.1e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write(("\n" if a.append else "") + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
