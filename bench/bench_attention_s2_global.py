"""Global attention on the sphere: the ``attention_s2_global`` op against the two routes a user has without it, in
one process on the same inputs:

  (a) the ``attention_s2`` op (the windowed kernel) on a whole-sphere ``hw`` table, as a hipGraph like ours;
  (b) ``torch.nn.functional.scaled_dot_product_attention`` on the flattened [B, heads, N, d] tensors (made contiguous
      outside the timed region) with the ``logw`` bias as ``attn_mask``, timed EAGERLY, one call per round.

  python bench/bench_attention_s2_global.py [--rounds 7] [--dtype both] [--out profiles/attention_s2_global_r19.txt]

Routes alternate round by round; median of the rounds with [min, max].  Per route the log gives us per call, the
(query, key) pairs per second and the MFMA FLOP/s that 4 d flops per pair imply."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensorrt_dft_plugins_amd as tdp  # noqa: E402
from bench.bench_disco import _rel, time_eager_once  # noqa: E402
from bench.bench_fft import time_graph  # noqa: E402
from tensorrt_dft_plugins_amd.ops import attention_s2 as A  # noqa: E402

HEADS = 4
# (key / value [B, C, nlat, nlon], out grid)
SHAPES = [((1, 128, 90, 180), (90, 180)), ((1, 256, 45, 90), (45, 90)), ((1, 128, 90, 180), (45, 90))]


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
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        if a.out:  # rewritten line by line: a run that ends early leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"Global attention on the sphere, equiangular grids, {HEADS} heads, median of {a.rounds} alternated rounds "
         f"[min, max]; us per call; global and windowed: hipGraph of {a.iters} calls; sdpa: eager, one call per round")
    emit(f"device: {torch.cuda.get_device_name(0)}")
    for shape, outs in SHAPES:
        torch.manual_seed(0)
        B, C, Hi, Wi = shape
        d = C // HEADS
        scale = d ** -0.5
        pairs = B * HEADS * Hi * Wi * outs[0] * outs[1]
        emit("")
        emit(f"{list(shape)} -> {list(outs)}, d = {d}: {pairs} pairs per call")
        t = A.attention_s2_global_table_holder((Hi, Wi), "equiangular", dev)
        hw = torch.full((outs[0], Hi), Wi // 2, dtype=torch.int32, device=dev)
        bias = t.logw.repeat_interleave(Wi)
        q32 = torch.randn(B, C, *outs, device=dev).to(bf).float()
        k32 = torch.randn(*shape, device=dev).to(bf).float()
        v32 = torch.randn(*shape, device=dev).to(bf).float()
        for dt in ([torch.float32, bf] if a.dtype == "both" else [torch.float32 if a.dtype == "fp32" else bf]):
            q, k, v = q32.to(dt), k32.to(dt), v32.to(dt)
            name = "fp32" if dt == torch.float32 else "bf16"
            emit(f" {name}  global: {ops.attention_s2_global_info(B, HEADS, d, Hi, Wi, outs[0], outs[1], dt == bf)}")
            emit(f"       windowed: {ops.attention_s2_info(B, HEADS, d, Hi, Wi, outs[0], outs[1], dt == bf)}")
            qs, ks, vs = (x.reshape(B, HEADS, d, -1).transpose(-1, -2).contiguous() for x in (q, k, v))
            mask = bias.to(dt)[None, None, None, :]
            routes = {
                "global": lambda: ops.attention_s2_global(q, k, v, t.logw, HEADS, scale),
                "windowed": lambda: ops.attention_s2(q, k, v, hw, t.logw, HEADS, scale),
                "sdpa eager": lambda: F.scaled_dot_product_attention(qs, ks, vs, attn_mask=mask, scale=scale)
                .transpose(-1, -2).reshape(q.shape),
            }
            with torch.no_grad():
                ref = routes["global"]()
                diffs = {n: _rel(fn(), ref) for n, fn in routes.items() if n != "global"}
                ts = {n: [] for n in routes}
                for _ in range(a.rounds):
                    for n, fn in routes.items():
                        ts[n].append(time_eager_once(fn) if n == "sdpa eager" else time_graph(fn, a.iters))
            mg = statistics.median(ts["global"])
            for n, tn in ts.items():
                m = statistics.median(tn)
                emit(f"  {n:<10} {m:10.1f} us [{min(tn):.1f}, {max(tn):.1f}]  {pairs / m / 1e3:8.1f} G pairs/s "
                     f"{4.0 * d * pairs / m / 1e6:7.2f} TFLOP/s"
                     + ("" if n == "global" else f"  / global {m / mg:.2f}  rel diff to global {diffs[n]:.1e}"))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
