"""The ``disco_t`` kernel (csrc/spectral/disco_t.hip) and ``DiscreteContinuousConvTransposeS2`` on the GPU, under
``strict_mode`` with no fallback counted.

Kernel cases (planes, in grid -> out grid, basis), each ragged against the instance's tiles:

* ``t1``   1 plane, (13, 24) -> (13, 24), nr = 3: PT = 1, s = 1, one partly filled slice of 256 lanes;
* ``t5``   5 planes, (9, 16) -> (17, 32), (3, 4): PT = 4 with a tile of one plane, s = 2, K = 9;
* ``t17``  17 planes, (9, 80) -> (17, 160), nr = 2: PT = 4, nlon_in above a wave's 64 lanes and no multiple of 64;
* ``pass`` 5 planes, (9, 200) -> (9, 200), nr = 2: PT = 4, 800 lanes' worth of outputs per phase, two passes of 768
  (at nlon_in = 360 an LDS row of K * nlon_in * 4 bytes no longer leaves PT = 4 its eight rows, and PT = 1 has one
  pass: 200 is the width that keeps both);
* ``ph``   2 planes, (5, 64) -> (9, 2048), nr = 2: PT = 1, 32 phases;
* ``ch1``  2 planes, (12, 2048) -> (12, 2048), nr = 2: PT = 1, a chunk of 4 input latitudes against taller bands,
  three passes, each re-staging its chunks;
* ``ch4``  5 planes, (20, 240) -> (20, 480), nr = 2, theta_cutoff = 6 pi / 19: PT = 4, a chunk of 8 against bands
  above 8, two passes.

Every case runs in fp32 and bf16, which are the four instances (2 dtypes x PT in {1, 4}), with and without bias.

Elementwise bound, from the dot product's error bound for any summation order plus the bias add: ref is the fp64 sum
of the same fp32 ``val`` and the same z (the CPU op's fp64 form) plus the bias, n_e the entry count of the output's
row: fp32 |y - ref| <= 1.01 (n_e + 1) 2^-24 (sum |val| |z| + |bias|); bf16 that plus 2^-8 |ref|.
Module: per field against the fp64 torch backend, fp32 < 1e-5 (``fno_pointwise`` is a bf16x3 split, the bound of
tests/test_disco_gpu.py), bf16 < 2e-2; the encoder-decoder pair is held to the same two bounds."""
import math
import re

import numpy as np
import pytest
import torch

from test_kernel_bounds_gpu import Guarded, _check_untouched
from tensorrt_dft_plugins_amd import utils
from tensorrt_dft_plugins_amd.models import DiscreteContinuousConvS2, DiscreteContinuousConvTransposeS2
from tensorrt_dft_plugins_amd.ops import disco as D
from tensorrt_dft_plugins_amd.ops import spectral as SP

ops = torch.ops.amd_dft
BF = torch.bfloat16

# name -> (planes, in_shape, out_shape, kernel_shape, theta_cutoff, (PT, passes), chunked)
CASES = {
    "t1": (1, (13, 24), (13, 24), 3, None, (1, 1), False),
    "t5": (5, (9, 16), (17, 32), (3, 4), None, (4, 1), False),
    "t17": (17, (9, 80), (17, 160), 2, None, (4, 1), False),
    "pass": (5, (9, 200), (9, 200), 2, None, (4, 2), False),
    "ph": (2, (5, 64), (9, 2048), 2, None, (1, 1), False),
    "ch1": (2, (12, 2048), (12, 2048), 2, None, (1, 3), True),
    "ch4": (5, (20, 240), (20, 480), 2, 6.0 * math.pi / 19.0, (4, 2), True),
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


_TABLES = {}


def _tables(name):
    if name not in _TABLES:
        _, ins, outs, ks, cut, _, _ = CASES[name]
        _TABLES[name] = tuple(torch.from_numpy(a) for a in D.disco_transpose_tables(ins, outs, ks, theta_cutoff=cut))
    return _TABLES[name]


def _tallest_band(name):
    """The most input latitudes any output latitude's s rows touch, from the table itself."""
    _, ins, outs, ks, _, _, _ = CASES[name]
    rp, idx, _ = _tables(name)
    s = outs[1] // ins[1]
    kin = idx.long() // (D.kernel_size(ks) * ins[1])
    return max(int(kin[rp[k * s]:rp[(k + 1) * s]].max() - kin[rp[k * s]:rp[(k + 1) * s]].min()) + 1
               for k in range(outs[0]) if rp[(k + 1) * s] > rp[k * s])


_REFS = {}


def _case(name, prec):
    """(z on the CPU in the case's dtype, bias fp32, K, fp64 ref without bias, fp64 sum |val||z|, n_e per output
    [Ho, Wo]), built once and left unchanged."""
    key = (name, prec)
    if key not in _REFS:
        planes, ins, outs, ks, _, _, _ = CASES[name]
        K = D.kernel_size(ks)
        rp, idx, val = _tables(name)
        s = outs[1] // ins[1]
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        z = torch.randn(planes, K, *ins, generator=g).to(BF if prec == "bf16" else torch.float32)
        bias = torch.randn(planes, generator=g)
        ref = ops.disco_t(z.double(), rp, idx, val.double(), *outs)
        mag = ops.disco_t(z.double().abs(), rp, idx, val.double(), *outs)
        n_e = torch.from_numpy(np.diff(rp.numpy())).double().reshape(outs[0], 1, s).expand(outs[0], ins[1], s)
        _REFS[key] = (z, bias, K, ref, mag, n_e.reshape(outs[0], outs[1]))
    return _REFS[key]


def _check(y, name, prec, with_bias, what):
    _, bias, _, ref, mag, n_e = _case(name, prec)
    if with_bias:
        b = bias.double()[:, None, None]
        ref, mag = ref + b, mag + b.abs()
    err = (y.detach().cpu().double() - ref).abs()
    bound = 1.01 * (n_e + 1.0) * 2.0 ** -24 * mag
    if prec == "bf16":
        bound = bound + 2.0 ** -8 * ref.abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"MEASURED disco_t {what} {name} {prec} bias={int(with_bias)} max |err| {float(err.max()):.3e} "
          f"worst err/bound {worst:.3f}")
    assert bool((err <= bound).all())


def test_every_shipped_instance_and_edge_is_reached():
    """Host only: the (PT, dtype) instances and the edges, from ``disco_t_info`` and the tables' own bands."""
    seen, phases, chunked_pt = set(), set(), set()
    for name, (planes, ins, outs, ks, _, (pt, passes), chunked) in CASES.items():
        K = D.kernel_size(ks)
        nnz = len(_tables(name)[1])
        band = _tallest_band(name)
        for bf in (False, True):
            f = _fields(ops.disco_t_info(planes, *ins, K, *outs, nnz, bf))
            assert (f["PT"], f["passes"]) == (pt, passes), (name, f)
            assert planes % f["PT"] or f["PT"] == 1, name   # a ragged plane tile
            # a partly filled slice of lanes, except ch1: 2048 lanes are eight full slices (three passes of 768, the
            # last one with two slices)
            assert bool((f["PT"] * ins[1]) % 256) == (name != "ch1"), name
            assert f["lds"] <= 64 * 1024 and f["wgs"] == outs[0] * -(-planes // f["PT"])
            assert f["phases"] == outs[1] // ins[1] and f["lds"] == f["PT"] * f["rows"] * K * ins[1] * 4
            assert (band > f["rows"]) == chunked, (name, band, f)
            if chunked:
                chunked_pt.add(f["PT"])
            seen.add((f["PT"], bf))
            phases.add(f["phases"])
    assert seen == {(1, False), (1, True), (4, False), (4, True)}
    assert chunked_pt == {1, 4}
    assert 1 in phases and 2 in phases and max(phases) >= 3
    assert any(c[1][1] > 64 and c[1][1] % 64 for c in CASES.values())
    assert any(c[5][1] == 2 for c in CASES.values())
    assert (_fields(ops.disco_t_info(2, 12, 2048, 2, 12, 2048, 1, False))["rows"],
            _fields(ops.disco_t_info(5, 20, 240, 2, 20, 480, 1, False))["rows"]) == (4, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(CASES))
def test_disco_t_elementwise(device, strict, name, prec, with_bias):
    z, bias, _, ref, _, _ = _case(name, prec)
    outs = CASES[name][2]
    y = ops.disco_t(z.to(device), *(t.to(device) for t in _tables(name)), *outs,
                    bias.to(device) if with_bias else None)
    assert y.dtype == z.dtype and y.shape == ref.shape
    _check(y, name, prec, with_bias, "kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["t5", "t17", "ph", "ch1", "ch4"])
def test_disco_t_out_guard_bands_odd_offset_and_stale_lds(device, strict, name, prec):
    """``disco_t_out`` with every tensor between NaN guard bands, z one element off the 16-byte boundary, launched
    right after ``lds_poison()``: finite, within the bound, guards and inputs bitwise unchanged."""
    z, bias, _, ref, _, _ = _case(name, prec)
    rp, idx, val = _tables(name)
    outs = CASES[name][2]
    gz = Guarded(device, 0, z, offset=1)
    gv = Guarded(device, 1, val, offset=3)
    gb = Guarded(device, 3, bias, offset=1)
    # the integer tables between guards of their own pattern
    pad = torch.full((4096,), 0x7FFFFFFF, dtype=torch.int32)
    rb, ib = torch.cat([pad, rp, pad]).to(device), torch.cat([pad, idx, pad]).to(device)
    rv, iv = rb[4096:4096 + len(rp)], ib[4096:4096 + len(idx)]
    gy = Guarded(device, 2, shape=tuple(ref.shape), dtype=z.dtype, offset=1)
    assert gz.view.data_ptr() % 16 != 0
    ops.disco_t_out(gz.view, rv, iv, gv.view, *outs, gb.view, gy.view)  # first call: nothing is built between poison and run
    torch.cuda.synchronize()
    gy.bits.fill_(gy.pattern)
    ops.lds_poison()
    assert float(ops.lds_probe()) == 1.0
    ops.lds_poison()
    assert ops.disco_t_out(gz.view, rv, iv, gv.view, *outs, gb.view, gy.view) is gy.view
    _check_untouched([gz, gv, gb], gy)
    assert torch.equal(rb.cpu(), torch.cat([pad, rp, pad])) and torch.equal(ib.cpu(), torch.cat([pad, idx, pad]))
    _check(gy.view, name, prec, True, "guarded")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(CASES))
def test_disco_t_bitwise_runs_graph_and_roll(device, strict, name, prec):
    z, bias, _, _, _, _ = _case(name, prec)
    _, ins, outs, _, _, _, _ = CASES[name]
    s = outs[1] // ins[1]
    zd, bd = z.to(device), bias.to(device)
    td = tuple(t.to(device) for t in _tables(name))
    a = ops.disco_t(zd, *td, *outs, bd)
    b = ops.disco_t(zd, *td, *outs, bd)
    assert torch.equal(a, b)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.disco_t(zd, *td, *outs, bd)
    torch.cuda.current_stream().wait_stream(stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = ops.disco_t(zd, *td, *outs, bd)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, a)
    # each output sums its row in table order wherever it sits on the row: the roll is exact
    for t in (1, 7):
        assert torch.equal(ops.disco_t(torch.roll(zd, t, dims=-1), *td, *outs, bd), torch.roll(a, s * t, dims=-1))


_MODS = {}
_MOD_CFGS = [((9, 16), (17, 32), (3, 4), "equiangular", "equiangular"),
             ((6, 12), (12, 36), 2, "legendre-gauss", "legendre-gauss"),
             ((17, 32), (33, 64), 3, "legendre-gauss", "equiangular")]


def _module(cfg):
    """(module on the CPU, x fp32 rounded to bf16 values, fp64 torch-backend reference), built once."""
    if cfg not in _MODS:
        ins, outs, ks, gi, go = cfg
        torch.manual_seed(21)
        m = DiscreteContinuousConvTransposeS2(5, 7, ins, outs, ks, grid_in=gi, grid_out=go).eval()
        with torch.no_grad():
            m.bias.normal_()
            x = torch.randn(2, 5, *ins).to(BF).float()
            ref = m.set_backend("torch")(x.double())
        _MODS[cfg] = (m.set_backend("amd"), x, ref)
    return _MODS[cfg]


def _field_err(out, ref):
    o, r = out.cpu().double().flatten(2), ref.flatten(2)
    return float(((o - r).norm(dim=2) / r.norm(dim=2)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cfg", _MOD_CFGS, ids=["eq-s2-3x4", "lg-s3-nr2", "lg-eq-s2-nr3"])
def test_module_vs_fp64_torch_backend(device, strict, cfg, prec):
    m, x, ref = _module(cfg)
    m = m.to(device)
    try:
        with torch.no_grad():
            out = m(x.to(device).to(BF if prec == "bf16" else torch.float32))
    finally:
        m.to("cpu")
    assert out.dtype == (BF if prec == "bf16" else torch.float32) and out.shape == ref.shape
    err = _field_err(out, ref)
    print(f"MEASURED disco_t module {cfg[0]}->{cfg[1]} {prec} per-field rel-L2 {err:.3e}")
    assert err < (2e-2 if prec == "bf16" else 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_encoder_decoder_pair(device, strict, prec):
    """``DiscreteContinuousConvS2`` to the coarse grid, ``DiscreteContinuousConvTransposeS2`` back to the input
    grid."""
    fine, coarse, ks = (17, 32), (9, 16), (3, 4)
    torch.manual_seed(22)
    m = torch.nn.Sequential(DiscreteContinuousConvS2(5, 7, fine, coarse, ks),
                            DiscreteContinuousConvTransposeS2(7, 5, coarse, fine, ks)).eval()
    with torch.no_grad():
        m[0].bias.normal_()
        m[1].bias.normal_()
        x = torch.randn(2, 5, *fine).to(BF).float()
        ref = m[1].set_backend("torch")(m[0].set_backend("torch")(x.double()))
        m[0].set_backend("amd")
        m[1].set_backend("amd")
        out = m.to(device)(x.to(device).to(BF if prec == "bf16" else torch.float32))
    assert out.shape == x.shape
    err = _field_err(out, ref)
    print(f"MEASURED disco_t encoder-decoder {prec} per-field rel-L2 {err:.3e}")
    assert err < (2e-2 if prec == "bf16" else 1e-5)
