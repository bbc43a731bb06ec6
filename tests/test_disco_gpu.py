"""The ``disco`` kernel (csrc/spectral/disco.hip) and ``DiscreteContinuousConvS2`` on the GPU, under ``strict_mode``
with no fallback counted.

Kernel cases (planes, in grid, out grid, basis), each ragged against the instance's tiles:

* ``p1``   1 plane, (13, 24) -> (13, 24): PT = 1, one partly filled slice of 256 lanes;
* ``p5``   5 planes, (17, 32) -> (9, 16), s = 2, anisotropic: PT = 4 with a tile of one plane;
* ``p17``  17 planes, (9, 160) -> (9, 160): PT = 4, nlon_out above a wave's 64 lanes and no multiple of 64;
* ``pass`` 5 planes, (9, 360) -> (9, 360): PT = 4, 1440 outputs per workgroup, two passes of 768;
* ``ch1``  2 planes, (40, 2048) -> (5, 64), s = 32: PT = 1, bands of 30 and more rows against a chunk of 8;
* ``ch4``  5 planes, (20, 480) -> (3, 120), s = 4: PT = 4, bands of 20 rows against a chunk of 8.

Every case runs in fp32 and bf16, which are the four instances (2 dtypes x PT in {1, 4}).

Elementwise bound, from the dot product's error bound for any summation order: ref is the fp64 sum of the same fp32
``val`` and the same x (the CPU op's fp64 form), n_e the entry count of the output's row:
fp32 |y - ref| <= 1.01 n_e 2^-24 sum |val| |x|; bf16 that plus 2^-8 |ref|.
Module: per field against the fp64 torch backend, fp32 < 1e-5 (``fno_pointwise`` is a bf16x3 split, the bound of
tests/test_sht_gpu.py), bf16 < 2e-2."""
import re

import numpy as np
import pytest
import torch

from test_kernel_bounds_gpu import Guarded, _check_untouched
from tensorrt_dft_plugins_amd import utils
from tensorrt_dft_plugins_amd.models import DiscreteContinuousConvS2
from tensorrt_dft_plugins_amd.ops import disco as D
from tensorrt_dft_plugins_amd.ops import spectral as SP

ops = torch.ops.amd_dft
BF = torch.bfloat16

# name -> (planes, in_shape, out_shape, kernel_shape, (PT, passes), chunked)
CASES = {
    "p1": (1, (13, 24), (13, 24), 3, (1, 1), False),
    "p5": (5, (17, 32), (9, 16), (3, 4), (4, 1), False),
    "p17": (17, (9, 160), (9, 160), 2, (4, 1), False),
    "pass": (5, (9, 360), (9, 360), 2, (4, 2), False),
    "ch1": (2, (40, 2048), (5, 64), 2, (1, 1), True),
    "ch4": (5, (20, 480), (3, 120), 2, (4, 1), True),
}
PRECS = ["fp32", "bf16"]


@pytest.fixture()
def strict():
    prev = utils.strict_mode(True)
    SP.fallback_reset()
    try:
        yield
        assert SP.fallback_counts() == {}
    finally:
        utils.strict_mode(prev)


def _fields(info):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", info)}


_REFS = {}


def _case(name, prec):
    """(x on the CPU in the case's dtype, CPU tables, K, fp64 ref, fp64 sum |val||x|, n_e per row [K, Ho, 1]), built
    once and left unchanged."""
    key = (name, prec)
    if key not in _REFS:
        planes, ins, outs, ks, _, _ = CASES[name]
        K = D.kernel_size(ks)
        rp, idx, val = (torch.from_numpy(a) for a in D.disco_tables(ins, outs, ks))
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        x = torch.randn(planes, *ins, generator=g).to(BF if prec == "bf16" else torch.float32)
        ref = ops.disco(x.double(), rp, idx, val.double(), K, *outs)
        mag = ops.disco(x.double().abs(), rp, idx, val.double(), K, *outs)
        n_e = torch.from_numpy(np.diff(rp.numpy())).double().reshape(K, outs[0], 1)
        _REFS[key] = (x, (rp, idx, val), K, ref, mag, n_e)
    return _REFS[key]


def _bound(prec, ref, mag, n_e):
    b = 1.01 * n_e * 2.0 ** -24 * mag
    return b + 2.0 ** -8 * ref.abs() if prec == "bf16" else b


def _check(y, name, prec, what):
    _, _, _, ref, mag, n_e = _case(name, prec)
    err = (y.detach().cpu().double() - ref).abs()
    bound = _bound(prec, ref, mag, n_e)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"MEASURED disco {what} {name} {prec} max |err| {float(err.max()):.3e} worst err/bound {worst:.3f}")
    assert bool((err <= bound).all())


def test_every_shipped_instance_is_reached():
    """Host only: the (PT, dtype) instances, a second pass, and the chunk of the two chunked cases."""
    seen = set()
    for name, (planes, ins, outs, ks, (pt, passes), chunked) in CASES.items():
        nnz = len(D.disco_tables(ins, outs, ks)[1]) if not chunked else 1
        for bf in (False, True):
            f = _fields(ops.disco_info(planes, *ins, D.kernel_size(ks), *outs, nnz, bf))
            assert (f["PT"], f["passes"]) == (pt, passes), (name, f)
            assert planes % f["PT"] or f["PT"] == 1, name  # a ragged plane tile
            assert (f["PT"] * outs[1]) % 256, name          # a partly filled slice of lanes
            assert f["lds"] <= 64 * 1024 and f["wgs"] == outs[0] * -(-planes // f["PT"])
            if chunked:
                assert f["rows"] < ins[0]  # the GPU test checks the bands of the table against it
            seen.add((f["PT"], bf))
    assert seen == {(1, False), (1, True), (4, False), (4, True)}
    assert any(c[1][1] > 64 and c[1][1] % 64 for c in CASES.values())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(CASES))
def test_disco_elementwise(device, strict, name, prec):
    x, tables, K, ref, _, _ = _case(name, prec)
    outs = CASES[name][2]
    if CASES[name][5]:  # chunked: some band really is taller than the chunk
        rp, idx, _ = tables
        f = _fields(ops.disco_info(x.shape[0], *CASES[name][1], K, *outs, len(idx), prec == "bf16"))
        rows_of = idx.long() // CASES[name][1][1]
        band = max(int(rows_of[rp[r]:rp[r + 1]].max() - rows_of[rp[r]:rp[r + 1]].min()) + 1
                   for r in range(K * outs[0]) if rp[r + 1] > rp[r])
        assert band > f["rows"], (band, f)
    y = ops.disco(x.to(device), *(t.to(device) for t in tables), K, *outs)
    assert y.dtype == x.dtype and y.shape == ref.shape
    _check(y, name, prec, "kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["p5", "p17", "ch1", "ch4"])
def test_disco_out_guard_bands_odd_offset_and_stale_lds(device, strict, name, prec):
    """``disco_out`` with every tensor between NaN guard bands, x one element off the 16-byte boundary, launched
    right after ``lds_poison()``: finite, within the bound, guards and inputs bitwise unchanged."""
    x, (rp, idx, val), K, ref, _, _ = _case(name, prec)
    outs = CASES[name][2]
    gx = Guarded(device, 0, x, offset=1)
    gv = Guarded(device, 1, val, offset=3)
    # the integer tables between guards of their own pattern
    pad = torch.full((4096,), 0x7FFFFFFF, dtype=torch.int32)
    rb, ib = torch.cat([pad, rp, pad]).to(device), torch.cat([pad, idx, pad]).to(device)
    rv, iv = rb[4096:4096 + len(rp)], ib[4096:4096 + len(idx)]
    gy = Guarded(device, 2, shape=tuple(ref.shape), dtype=x.dtype, offset=1)
    assert gx.view.data_ptr() % 16 != 0
    ops.disco_out(gx.view, rv, iv, gv.view, K, *outs, gy.view)  # first call: nothing is built between poison and run
    torch.cuda.synchronize()
    gy.bits.fill_(gy.pattern)
    ops.lds_poison()
    assert float(ops.lds_probe()) == 1.0
    ops.lds_poison()
    assert ops.disco_out(gx.view, rv, iv, gv.view, K, *outs, gy.view) is gy.view
    _check_untouched([gx, gv], gy)
    assert torch.equal(rb.cpu(), torch.cat([pad, rp, pad])) and torch.equal(ib.cpu(), torch.cat([pad, idx, pad]))
    _check(gy.view, name, prec, "guarded")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["p5", "p17", "ch4"])
def test_disco_bitwise_runs_graph_and_roll(device, strict, name, prec):
    x, tables, K, _, _, _ = _case(name, prec)
    _, ins, outs, _, _, _ = CASES[name]
    s = ins[1] // outs[1]
    xd = x.to(device)
    td = tuple(t.to(device) for t in tables)
    a = ops.disco(xd, *td, K, *outs)
    b = ops.disco(xd, *td, K, *outs)
    assert torch.equal(a, b)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.disco(xd, *td, K, *outs)
    torch.cuda.current_stream().wait_stream(stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = ops.disco(xd, *td, K, *outs)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, a)
    # each output sums its row in table order wherever it sits on the row: the roll is exact
    for t in (1, 7):
        assert torch.equal(ops.disco(torch.roll(xd, s * t, dims=-1), *td, K, *outs), torch.roll(a, t, dims=-1))


_MODS = {}


def _module(cfg):
    """(module on the CPU, x fp32 rounded to bf16 values, fp64 torch-backend reference), built once."""
    if cfg not in _MODS:
        ins, outs, ks, gi, go = cfg
        torch.manual_seed(21)
        m = DiscreteContinuousConvS2(5, 7, ins, outs, ks, grid_in=gi, grid_out=go).eval()
        with torch.no_grad():
            m.bias.normal_()
            x = torch.randn(2, 5, *ins).to(BF).float()
            ref = m.set_backend("torch")(x.double())
        _MODS[cfg] = (m.set_backend("amd"), x, ref)
    return _MODS[cfg]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cfg", [((17, 32), (9, 16), (3, 4), "equiangular", "equiangular"),
                                 ((12, 36), (6, 12), 2, "legendre-gauss", "legendre-gauss"),
                                 ((33, 64), (33, 64), 3, "equiangular", "legendre-gauss")],
                         ids=["eq-s2-3x4", "lg-s3-nr2", "eq-lg-s1-nr3"])
def test_module_vs_fp64_torch_backend(device, strict, cfg, prec):
    m, x, ref = _module(cfg)
    m = m.to(device)
    try:
        with torch.no_grad():
            out = m(x.to(device).to(BF if prec == "bf16" else torch.float32))
    finally:
        m.to("cpu")
    assert out.dtype == (BF if prec == "bf16" else torch.float32) and out.shape == ref.shape
    o, r = out.cpu().double().flatten(2), ref.flatten(2)
    err = float(((o - r).norm(dim=2) / r.norm(dim=2)).max())
    print(f"MEASURED disco module {cfg[0]}->{cfg[1]} {prec} per-field rel-L2 {err:.3e}")
    assert err < (2e-2 if prec == "bf16" else 1e-5)
