"""The ``disco_spectral`` kernel (csrc/spectral/disco_spectral.hip) and ``DiscreteContinuousConvS2`` with
``algorithm="spectral"`` on the GPU, under ``strict_mode`` with no fallback counted.

Op cases: the six shapes of tests/test_disco_spectral.py (``m17``: 17 modes against a tile of 8) with 1, 5 and 17
planes (a ragged plane tile, and two tiles), plus three with s = 8, 16, 32 (U = 14), whose long contractions reach
the other instances: ``kd224`` (fp32 8 modes x 8 planes), ``kd448`` (fp32 4 x 8, bf16 8 x 8), ``kd896`` (bf16 4 x 8;
fp32 does not fit 64 KiB and raises).

Reference: the fp64 CPU op on the same xhat and the same rounded table.  fp32: per-field rel-L2 < 1e-5, the project's
bound for its bf16x3 kernels (tests/test_sht_gpu.py), on every case.  bf16: every element within
2^-8 |ref| + KD 2^-22 sum |t| |x| (``legendre`` / ``sfno_mix``; KD the padded contraction).
Module: per field against the fp64 torch backend, fp32 < 1e-5 and bf16 < 2e-2, as tests/test_disco_gpu.py."""
import re

import pytest
import torch

import test_disco_gpu as GATHER
from test_disco_gpu import strict  # noqa: F401  (fixture)
from test_disco_spectral import SHAPES
from test_kernel_bounds_gpu import Guarded, _check_untouched
from tensorrt_dft_plugins_amd.models import DiscreteContinuousConvS2
from tensorrt_dft_plugins_amd.ops import disco as D

ops = torch.ops.amd_dft
BF, PRECS = torch.bfloat16, GATHER.PRECS
# name -> (in_shape, out_shape, kernel_shape, grid, {prec: (MT, PTL)})
CASES = {n: (*c, {"fp32": (8, 16), "bf16": (8, 16)}) for n, c in SHAPES.items()}
CASES["kd224"] = ((17, 64), (9, 8), (2, 3), "equiangular", {"fp32": (8, 8), "bf16": (8, 16)})
CASES["kd448"] = ((17, 128), (9, 8), (2, 3), "equiangular", {"fp32": (4, 8), "bf16": (8, 8)})
CASES["kd896"] = ((17, 256), (9, 8), (2, 3), "equiangular", {"bf16": (4, 8)})
RUNS = [(n, p) for n in SHAPES for p in (1, 5, 17)] + [("kd224", 17), ("kd448", 17), ("kd896", 9)]

_REFS = {}


def _case(name, planes, prec):
    """(xhat on the CPU in the case's dtype, holder, table of the precision, op arguments from lo on, fp64 ref, fp64
    sum |t| |x|), built once and left unchanged."""
    key = (name, planes, prec)
    if key not in _REFS:
        ins, outs, ks, grid, _ = CASES[name]
        h = D.disco_spectral_table_holder(ins, outs, ks, grid, grid)
        g = torch.Generator().manual_seed(planes + sum(map(ord, name)))
        xh = torch.randn(planes, ins[0], ins[1] // 2 + 1, 2, generator=g).to(BF if prec == "bf16" else torch.float32)
        table = h.table_bf16 if prec == "bf16" else h.table
        args = (h.lo, h.K, h.U, outs[0], ins[1], outs[1])
        ref = ops.disco_spectral(xh.double(), table, *args)
        # sum |t| |x|: (|xr|, 0) and (|xi|, 0) against (|Re t|, |Im t|), whose real and imaginary parts are the four sums
        z = torch.zeros_like(xh[..., 0], dtype=torch.float64)
        a = ops.disco_spectral(torch.stack([xh[..., 0].double().abs(), z], -1), table.abs(), *args)
        b = ops.disco_spectral(torch.stack([xh[..., 1].double().abs(), z], -1), table.abs(), *args)
        mag = torch.stack([a[..., 0] + b[..., 1], b[..., 0] + a[..., 1]], -1)
        _REFS[key] = (xh, h, table, args, ref, mag)
    return _REFS[key]


def _check(y, name, planes, prec, what):
    _, h, _, _, ref, mag = _case(name, planes, prec)
    yd = y.detach().cpu().double()
    rel = float(((yd - ref).flatten(2).norm(dim=2) / ref.flatten(2).norm(dim=2).clamp_min(1e-300)).max())
    worst = float(((yd - ref).abs() / (2.0 ** -8 * ref.abs() + h.KD * 2.0 ** -22 * mag).clamp_min(1e-300)).max())
    print(f"MEASURED disco_spectral {what} {name} planes {planes} {prec} per-field rel-L2 {rel:.3e} "
          f"worst err/bf16-bound {worst:.3f}")
    assert y.dtype == (BF if prec == "bf16" else torch.float32) and y.shape == ref.shape
    assert worst <= 1.0 if prec == "bf16" else rel < 1e-5


def _route(name, planes, prec):
    h = _case(name, planes, prec)[1]
    info = ops.disco_spectral_info(planes, *CASES[name][0], h.K, *CASES[name][1], h.U, prec == "bf16")
    return tuple(int(v) for v in re.search(r"MT=(\d+) PTL=(\d+)", info).groups())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,planes", RUNS)
def test_op_against_the_fp64_cpu_op(device, strict, name, planes, prec):  # noqa: F811
    if prec not in CASES[name][4]:
        xh, h, table, args, _, _ = _case(name, planes, "bf16")
        with pytest.raises(RuntimeError, match="bytes of LDS"):
            ops.disco_spectral(xh.float().to(device), h.table.to(device), args[0].to(device), *args[1:])
        return
    xh, _, table, args, _, _ = _case(name, planes, prec)
    assert _route(name, planes, prec) == CASES[name][4][prec]
    y = ops.disco_spectral(xh.to(device), table.to(device), args[0].to(device), *args[1:])
    _check(y, name, planes, prec, "kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,planes", [("k9", 5), ("s3", 17), ("odd", 5), ("kd448", 17)])
def test_out_guard_bands_poisoned_lo_bitwise_runs_and_graph(device, strict, name, planes, prec):  # noqa: F811
    """``disco_spectral_out`` with xhat, the table and the target between NaN guard bands (xhat and the target one
    pair off the 16-byte boundary), lo between rows of a poison that would index far outside xhat: guards and inputs
    bitwise unchanged, every element written and within the bound; a second run and a hipGraph replay are bitwise
    equal.  Then that poison inside lo, in its first and last entry: bitwise what lo clamped by hand gives, on the
    GPU and in the CPU op."""
    xh, _, table, args, ref, _ = _case(name, planes, prec)
    gx, gt = Guarded(device, 0, xh, offset=2), Guarded(device, 1, table)
    gy = Guarded(device, 2, shape=tuple(ref.shape), dtype=xh.dtype, offset=2)
    pad = torch.full((4096,), 0x7FFFFFFF, dtype=torch.int32)
    pad[::2] = -0x7FFFFFFF
    lb = torch.cat([pad, args[0], pad]).to(device)
    lo = lb[4096:4096 + len(args[0])]
    assert gx.view.data_ptr() % 16 != 0 and gy.view.data_ptr() % 16 != 0 and gt.view.data_ptr() % 16 == 0
    assert ops.disco_spectral_out(gx.view, gt.view, lo, *args[1:], gy.view) is gy.view
    _check_untouched([gx, gt], gy)
    assert torch.equal(lb.cpu(), torch.cat([pad, args[0], pad]))
    _check(gy.view, name, planes, prec, "guarded")
    first = gy.view.clone()
    assert torch.equal(ops.disco_spectral(gx.view, gt.view, lo, *args[1:]), first)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.disco_spectral(gx.view, gt.view, lo, *args[1:])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, first)
    bad = args[0].clone()
    bad[0], bad[-1] = -0x7FFFFFFF, 0x7FFFFFFF
    for x_, t_, d in ((gx.view, gt.view, device), (xh, table, "cpu")):
        yb, yc = (ops.disco_spectral(x_, t_, l.to(d), *args[1:]) for l in (bad, bad.clamp(0, xh.shape[1] - 1)))
        assert torch.equal(yb, yc) and not torch.equal(yb.cpu(), first.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cfg", [((17, 32), (9, 16), (3, 4), "equiangular", "equiangular"),
                                 ((12, 36), (6, 12), 2, "legendre-gauss", "legendre-gauss"),
                                 ((33, 64), (33, 64), 3, "equiangular", "legendre-gauss")],
                         ids=["eq-s2-3x4", "lg-s3-nr2", "eq-lg-s1-nr3"])
def test_module_vs_fp64_torch_backend(device, strict, cfg, prec):  # noqa: F811
    """The gather module's cases, inputs and fp64 reference (tests/test_disco_gpu.py), the same weights."""
    gather, x, ref = GATHER._module(cfg)
    ins, outs, ks, gi, go = cfg
    m = DiscreteContinuousConvS2(5, 7, ins, outs, ks, grid_in=gi, grid_out=go, algorithm="spectral").eval()
    m.load_state_dict(gather.state_dict())
    with torch.no_grad():
        out = m.to(device)(x.to(device).to(BF if prec == "bf16" else torch.float32))
    assert out.dtype == (BF if prec == "bf16" else torch.float32) and out.shape == ref.shape
    o, r = out.cpu().double().flatten(2), ref.flatten(2)
    err = float(((o - r).norm(dim=2) / r.norm(dim=2)).max())
    print(f"MEASURED disco_spectral module {cfg[0]}->{cfg[1]} {prec} per-field rel-L2 {err:.3e}")
    assert err < (2e-2 if prec == "bf16" else 1e-5)
