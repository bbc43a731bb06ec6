"""The ``disco_spectral_t`` op and ``DiscreteContinuousConvTransposeS2(algorithm="spectral")`` on the GPU, under
``strict_mode`` with no fallback counted: the shapes of tests/test_disco_spectral_t.py with 1, 5 and 17 planes (a
ragged plane tile, and two tiles), C = planes, with bias, against the fp64 CPU op on the same zhat, rounded table
and bias.  fp32: per-field rel-L2 < 1e-5, the project's bound for its bf16x3 kernels.  bf16: every element within
2^-8 |ref| + KD 2^-22 sum |t| |z|.  Module: per field against the fp64 torch backend, < 1e-5 and < 2e-2."""
import pytest
import torch

import test_disco_t_gpu as GATHER
from test_disco_t_gpu import strict  # noqa: F401  (fixture)
from test_disco_spectral_t import SHAPES
from test_kernel_bounds_gpu import Guarded, _check_untouched
from tensorrt_dft_plugins_amd.engine import Engine
from tensorrt_dft_plugins_amd.models import DiscreteContinuousConvTransposeS2
from tensorrt_dft_plugins_amd.ops import disco as D

ops = torch.ops.amd_dft
BF, PRECS = torch.bfloat16, GATHER.PRECS
_REFS = {}


def _case(name, planes, prec):
    """(zhat, table, op arguments lo .. nlon_out, bias, fp64 ref with the bias, fp64 sum |t| |z|, KD), built once."""
    key = (name, planes, prec)
    if key not in _REFS:
        ins, outs, ks, gi, go, cut, _ = SHAPES[name]
        h = D.disco_spectral_transpose_table_holder(ins, outs, ks, gi, go, cut)
        g = torch.Generator().manual_seed(planes + sum(map(ord, name)))
        zh = torch.randn(planes, h.K, ins[0], ins[1] // 2 + 1, 2, generator=g).to(BF if prec == "bf16" else torch.float32)
        bias = torch.randn(planes, generator=g)
        table = h.table_bf16 if prec == "bf16" else h.table
        args = (h.lo, h.K, h.U, outs[0], ins[1], outs[1])
        ref = ops.disco_spectral_t(zh.double(), table, *args, bias)
        # sum |t| |z|: (|zr|, 0) and (|zi|, 0) against (|Re t|, |Im t|), whose real and imaginary parts are the four sums
        z0 = torch.zeros_like(zh[..., 0], dtype=torch.float64)
        a = ops.disco_spectral_t(torch.stack([zh[..., 0].double().abs(), z0], -1), table.abs(), *args)
        b = ops.disco_spectral_t(torch.stack([zh[..., 1].double().abs(), z0], -1), table.abs(), *args)
        mag = torch.stack([a[..., 0] + b[..., 1], b[..., 0] + a[..., 1]], -1)
        _REFS[key] = (zh, table, args, bias, ref, mag, h.KD)
    return _REFS[key]


def _check(y, name, planes, prec, what):
    _, _, _, _, ref, mag, KD = _case(name, planes, prec)
    yd = y.detach().cpu().double()
    rel = float(((yd - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1).clamp_min(1e-300)).max())
    worst = float(((yd - ref).abs() / (2.0 ** -8 * ref.abs() + KD * 2.0 ** -22 * mag).clamp_min(1e-300)).max())
    print(f"MEASURED disco_spectral_t {what} {name} planes {planes} {prec} per-field rel-L2 {rel:.3e} "
          f"worst err/bf16-bound {worst:.3f}")
    assert y.dtype == (BF if prec == "bf16" else torch.float32) and y.shape == ref.shape
    assert worst <= 1.0 if prec == "bf16" else rel < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("planes", [1, 5, 17])
@pytest.mark.parametrize("name", list(SHAPES))
def test_op_against_the_fp64_cpu_op(device, strict, name, planes, prec):  # noqa: F811
    zh, table, args, bias, _, _, _ = _case(name, planes, prec)
    y = ops.disco_spectral_t(zh.to(device), table.to(device), args[0].to(device), *args[1:], bias.to(device))
    _check(y, name, planes, prec, "kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["k17", "kd128", "s3", "odd"])
def test_out_guard_bands_poisoned_lo_bitwise_runs_and_graph(device, strict, name, prec):  # noqa: F811
    """zhat and the target one pair off 16-byte alignment, lo between poison rows; then the poison inside lo, in its
    first and last entry: bitwise what lo clamped by hand gives, on the GPU and in the CPU op."""
    zh, table, args, bias, ref, _, _ = _case(name, 5, prec)
    gx, gt = Guarded(device, 0, zh, offset=2), Guarded(device, 1, table)
    gy = Guarded(device, 2, shape=tuple(ref.shape), dtype=zh.dtype, offset=2)
    pad = torch.tensor([-0x7FFFFFFF, 0x7FFFFFFF], dtype=torch.int32).repeat(2048)
    lb, bd = torch.cat([pad, args[0], pad]).to(device), bias.to(device)
    lo = lb[4096:4096 + len(args[0])]
    assert gx.view.data_ptr() % 16 != 0 and gy.view.data_ptr() % 16 != 0 and gt.view.data_ptr() % 16 == 0
    assert ops.disco_spectral_t_out(gx.view, gt.view, lo, *args[1:], bd, gy.view) is gy.view
    _check_untouched([gx, gt], gy)
    assert torch.equal(lb.cpu(), torch.cat([pad, args[0], pad])) and torch.equal(bd.cpu(), bias)
    _check(gy.view, name, 5, prec, "guarded")
    first, graph = gy.view.clone(), torch.cuda.CUDAGraph()
    assert torch.equal(ops.disco_spectral_t(gx.view, gt.view, lo, *args[1:], bd), first)
    with torch.cuda.graph(graph):
        y = ops.disco_spectral_t(gx.view, gt.view, lo, *args[1:], bd)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, first)
    bad = args[0].clone()
    bad[0], bad[-1] = -0x7FFFFFFF, 0x7FFFFFFF
    for x_, t_, b_, d in ((gx.view, gt.view, bd, device), (zh, table, bias, "cpu")):
        yb, yc = (ops.disco_spectral_t(x_, t_, l.to(d), *args[1:], b_) for l in (bad, bad.clamp(0, zh.shape[2] - 1)))
        assert torch.equal(yb, yc) and not torch.equal(yb.cpu(), first.cpu())


def _spectral(cfg, device):
    gather, x, ref = GATHER._module(cfg)  # the gather module's weights, input and fp64 reference
    m = DiscreteContinuousConvTransposeS2(5, 7, *cfg[:3], grid_in=cfg[3], grid_out=cfg[4], algorithm="spectral").eval()
    m.load_state_dict(gather.state_dict())
    return m.to(device), x.to(device), ref


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cfg", GATHER._MOD_CFGS, ids=["eq-s2-3x4", "lg-s3-nr2", "lg-eq-s2-nr3"])
def test_module_vs_fp64_torch_backend(device, strict, cfg, prec):  # noqa: F811
    m, x, ref = _spectral(cfg, device)
    with torch.no_grad():
        out = m(x.to(BF if prec == "bf16" else torch.float32))
    assert out.dtype == (BF if prec == "bf16" else torch.float32) and out.shape == ref.shape
    err = GATHER._field_err(out, ref)
    print(f"MEASURED disco_spectral_t module {cfg[0]}->{cfg[1]} {prec} per-field rel-L2 {err:.3e}")
    assert err < (2e-2 if prec == "bf16" else 1e-5)


@pytest.mark.gpu
def test_engine_builds_and_infers(device, strict):  # noqa: F811
    m, x, ref = _spectral(GATHER._MOD_CFGS[1], device)
    (y,) = Engine.build(m, (x,), device=device).infer(x)
    with torch.no_grad():
        assert torch.equal(y, m(x)) and GATHER._field_err(y, ref) < 1e-5
