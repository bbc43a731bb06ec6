"""The bf16 instances of the ``fno_mix`` kernels (csrc/spectral/fno_mix.hip) and the layers that run on them, on the
GPU, under ``strict_mode`` with no fallback counted.  Bounds and references: tests/test_fno_mix_bf16.py.

Kernel cases ``(B, Cin, Cout, M)``, the route of each asserted with ``fno_mix_info`` before it runs:

* ``stream``: every instance NB = 1 / 2 / 4 / 8 of both widths (``vec=2``, two modes per lane, for an even M; ``vec=1``
  for an odd one), B below NB, Cin < 4 (empty split-K ranges of some waves), odd Cin and Cout, M not a multiple of the
  64 outputs of a workgroup, M = 1; the odd-element and 4-mod-8 views send an even M to the one-mode instance too;
* ``mfma``: ragged batch rows (B % 16), K = 2 Cin not a multiple of 32, N = 2 Cout not a multiple of 16, M not a
  multiple of the mode tile and below it, exact-fit tiles, ``path=2`` at B = 2; and, since the fill rule gives every
  short spectrum the 4-mode tile, two narrow long ones that take the 8- and the 16-mode tile with a ragged last tile;
* ``stream-batched``: tiles beyond 160 KB, remainder launches of one and two samples, both widths.

Each case: the clean result within the elementwise and the per-field bound, twice with equal bits; ``fno_mix_out`` into
a guarded tensor with bands and inputs untouched; the same after every CU's LDS was filled with NaN; an x view at an
odd bf16 element; one hipGraph capture whose replay equals eager."""
import pytest
import torch

import test_fno_mix_bf16 as F
import test_sfno_bf16 as T
from test_kernel_bounds_gpu import Guarded, _check_untouched, _poison_then, lds
from tensorrt_dft_plugins_amd import utils
from tensorrt_dft_plugins_amd.engine import Engine
from tensorrt_dft_plugins_amd.models import SFNOConfig, SFNONet
from tensorrt_dft_plugins_amd.ops import spectral as SP

BF = torch.bfloat16
ops = torch.ops.amd_dft

# (B, Cin, Cout, M), path -> the head of fno_mix_info
CASES = {
    ((1, 20, 20, 100), 0): "stream NB=1 vec=2",
    ((2, 3, 5, 19), 0): "stream NB=2 vec=1",
    ((3, 7, 5, 130), 0): "stream NB=4 vec=2",
    ((5, 1, 1, 1), 0): "stream NB=8 vec=1",
    ((8, 20, 20, 65), 0): "stream NB=8 vec=1",
    ((1, 33, 2, 64), 0): "stream NB=1 vec=2",
    ((2, 5, 3, 6), 0): "stream NB=2 vec=2",
    ((7, 4, 4, 70), 0): "stream NB=8 vec=2",
    ((1, 3, 5, 131), 0): "stream NB=1 vec=1",
    ((4, 6, 3, 67), 0): "stream NB=4 vec=1",
    ((9, 20, 20, 37), 0): "mfma MT=4",
    ((12, 7, 5, 19), 0): "mfma MT=4",
    ((17, 16, 8, 8), 0): "mfma MT=4",
    ((32, 20, 20, 9), 0): "mfma MT=4",
    ((16, 1, 1, 3), 0): "mfma MT=4",
    ((2, 32, 16, 64), 2): "mfma MT=4",
    ((32, 48, 48, 6), 0): "mfma MT=4",  # 128 KB of LDS: beyond the 64 KB a kernel gets without asking
    ((9, 2, 2, 2051), 0): "mfma MT=8",
    ((9, 2, 2, 4099), 0): "mfma MT=16",
    ((9, 96, 96, 5), 0): "stream-batched NB=8 vec=1",
    ((17, 72, 40, 3), 0): "stream-batched NB=8 vec=1",
    ((10, 96, 96, 4), 0): "stream-batched NB=8 vec=2",
}
KEYS = list(CASES)
ids = lambda k: "x".join(map(str, k[0])) + (f"-path{k[1]}" if k[1] else "")  # noqa: E731


@pytest.fixture()
def strict():
    prev = utils.strict_mode(True)
    SP.fallback_reset()
    try:
        yield
        assert SP.fallback_counts() == {}
    finally:
        utils.strict_mode(prev)


def _route(key):
    (B, Cin, Cout, M), path = key
    s = ops.fno_mix_info(B, Cin, Cout, M, True, path)
    assert s.startswith(CASES[key] + " ") and s.endswith(" bf16=1"), s
    f = F.fields(s)
    assert f["launches"] == ((B + 7) // 8 if s.startswith("stream") else 1) and f["lds"] <= 160 * 1024
    return s


def _guarded(device, case):
    B, Cin, Cout, M = case
    x, _, wb, _, _ = F.fmix_case(case)
    return Guarded(device, 0, x), Guarded(device, 1, wb), Guarded(device, 2, shape=(B, Cout, M, 2), dtype=BF)


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS, ids=ids)
def test_fno_mix_bf16(device, strict, key):
    case, path = key
    _route(key)
    x, _, wb, _, _ = F.fmix_case(case)
    xd, wd = x.to(device), wb.to(device)
    out = ops.fno_mix(xd, wd, path)
    F.check_fmix(out, case, f"gpu path={path}")
    assert torch.equal(out, ops.fno_mix(xd, wd, path))
    if path == 0:
        assert torch.equal(out, SP.fno_spectral_mix(xd, wd))


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS, ids=ids)
def test_fno_mix_bf16_guard_bands(device, strict, key):
    case, path = key
    _route(key)
    gx, gw, gy = _guarded(device, case)
    assert ops.fno_mix_out(gx.view, gw.view, path, gy.view) is gy.view
    _check_untouched([gx, gw], gy)
    F.check_fmix(gy.view, case, "guarded")


@pytest.mark.gpu
@lds
@pytest.mark.parametrize("key", KEYS, ids=ids)
def test_fno_mix_bf16_stale_lds(device, strict, key):
    """Rows b >= B and n >= 2 Cout, the K padding and the modes past M of the MFMA tile must be written as zeros."""
    case, path = key
    gx, gw, gy = _guarded(device, case)
    _poison_then(lambda: ops.fno_mix_out(gx.view, gw.view, path, gy.view))
    ops.fno_mix_out(gx.view, gw.view, path, gy.view)
    _check_untouched([gx, gw], gy)
    F.check_fmix(gy.view, case, "stale-lds")


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS, ids=ids)
def test_fno_mix_bf16_view_at_odd_element(device, strict, key):
    case, path = key
    B, Cin, Cout, M = case
    x, _, wb, _, _ = F.fmix_case(case)
    bufs = []
    for t in (x, wb):
        buf = torch.zeros(t.numel() + 1, device=device, dtype=BF)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 4 == 2
        bufs.append(v)
    F.check_fmix(ops.fno_mix(bufs[0], bufs[1], path), case, "odd view")
    ybuf = torch.zeros(B * Cout * M * 2 + 2, device=device, dtype=BF)
    with pytest.raises(RuntimeError, match="4-byte"):
        ops.fno_mix_out(bufs[0], bufs[1], path, ybuf[1:-1].view(B, Cout, M, 2))
    y2 = ybuf[2:].view(B, Cout, M, 2)
    assert y2.data_ptr() % 8 == 4
    F.check_fmix(ops.fno_mix_out(x.to(device), wb.to(device), path, y2), case, "out at 4 mod 8")


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS, ids=ids)
def test_fno_mix_bf16_graph_replay(device, strict, key):
    case, path = key
    x, _, wb, _, _ = F.fmix_case(case)
    xd, wd = x.to(device), wb.to(device)
    eager = ops.fno_mix(xd, wd, path).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = ops.fno_mix(xd, wd, path)
    g.replay()
    torch.cuda.synchronize()
    assert y.dtype == BF and torch.equal(y, eager)


@pytest.mark.gpu
@pytest.mark.parametrize("key", [((3, 7, 5, 130), 0), ((12, 7, 5, 19), 0), ((20, 40, 40, 10), 0)], ids=ids)
def test_fno_mix_out_fp32_equals_the_op(device, strict, key):
    """The fp32 op is what it was; ``fno_mix_out`` is its launch path into the caller's tensor (8-byte aligned)."""
    case, path = key
    B, Cin, Cout, M = case
    assert ops.fno_mix_info(B, Cin, Cout, M, False, path).split()[0] == {3: "stream", 12: "mfma", 20: "stream-batched"}[B]
    x, w, _, _, yu = F.fmix_case(case)
    gx, gw = Guarded(device, 0, x.float()), Guarded(device, 1, w)
    gy = Guarded(device, 2, shape=(B, Cout, M, 2), dtype=torch.float32)
    assert ops.fno_mix_out(gx.view, gw.view, path, gy.view) is gy.view
    _check_untouched([gx, gw], gy)
    ref = ops.fno_mix(gx.view, gw.view, path)
    assert ref.dtype == torch.float32 and torch.equal(gy.view, ref)
    assert torch.equal(ops.fno_mix(x.to(device), w.to(device), path), ref)  # a mixed call: upcast, the fp32 kernels
    assert T.field_err(ref, yu, 2) < 1e-5
    ybuf = torch.zeros(B * Cout * M * 2 + 1, device=device)
    with pytest.raises(RuntimeError, match="8-byte"):
        ops.fno_mix_out(gx.view, gw.view, path, ybuf[1:].view(B, Cout, M, 2))


# ------------------------------------------------------------------------------------------------ layers
@pytest.mark.gpu
@pytest.mark.parametrize("operator,mix", [("diagonal", "auto"), ("dhconv", "expand")], ids=["diagonal", "expand"])
@pytest.mark.parametrize("shape,lmax,mmax,grid", T.SHT_CASES, ids=T.SHT_IDS)
def test_layers_on_fno_mix(device, strict, shape, lmax, mmax, grid, operator, mix, monkeypatch):
    """``SphericalConv2d`` / ``SFNOBlock`` with the per-mode operator, and with ``mix="expand"``, in fp32 and bf16:
    every mix call is ``fno_mix`` on tensors of the input's dtype, the result within the layer bound of the fp64 torch
    backend."""
    x, conv, blk, ref_c, ref_b = F.diag_refs(shape, lmax, mmax, grid, operator)
    conv.mix = blk.spectral.mix = mix
    calls = []
    F.spy_mix(monkeypatch, calls)
    conv, blk = conv.to(device), blk.to(device)
    with torch.no_grad():
        for dt, tol in ((torch.float32, 1e-5), (BF, T.TOL_LAYER)):
            xd = x.to(device).to(dt)
            out_c, out_b = conv(xd), blk(xd)
            assert out_c.shape == x.shape and out_c.dtype == dt and out_b.shape == x.shape and out_b.dtype == dt
            e_c, e_b = T.field_err(out_c, ref_c, 2), T.field_err(out_b, ref_b, 2)
            print(f"MEASURED sfno {operator} mix={mix} {shape} {dt} conv {e_c:.3e} block {e_b:.3e}")
            assert e_c < tol
            assert e_b < tol
    assert calls == [(torch.float32, torch.float32)] * 2 + [(BF, BF)] * 2


_NET = {}


def _net_and_ref():
    if not _NET:
        torch.manual_seed(12)
        net = SFNONet(SFNOConfig(img_size=(33, 64), in_chans=3, out_chans=3, embed_dim=16, depth=2,
                                 operator="diagonal")).eval()
        x = torch.randn(2, 3, 33, 64).to(BF)
        with torch.no_grad():
            for name, p in net.named_parameters():
                if "norm" in name:
                    p.copy_(1.0 + 0.3 * torch.randn_like(p) if name.endswith("weight") else 0.3 * torch.randn_like(p))
                p.copy_(p.to(BF).float())
            ref = net.set_backend("torch")(x.double())
        _NET["v"] = (net.set_backend("amd"), x, ref)
    return _NET["v"]


@pytest.mark.gpu
def test_sfno_net_diagonal_bf16_gpu(device, strict, monkeypatch):
    net, x, ref = _net_and_ref()
    calls = []
    F.spy_mix(monkeypatch, calls)
    net = net.to(device)
    try:
        with torch.no_grad():
            out = net(x.to(device))
    finally:
        net.cpu()
    assert out.dtype == BF and calls == [(BF, BF)] * 2
    err = T.field_err(out, ref, 2)
    print(f"MEASURED sfno_net diagonal bf16 gpu per-field rel-L2 {err:.3e}")
    assert err < T.TOL_LAYER


@pytest.mark.gpu
def test_sfno_net_diagonal_bf16_engine_gpu(device, strict):
    net, x, ref = _net_and_ref()
    xd = x.to(device)
    net = net.to(device)
    try:
        with torch.no_grad():
            eager = net(xd).clone()
    finally:
        net.cpu()
    eng = Engine.build(net, (x,), device=device, optimize=False)
    assert eng.use_graph
    (y,) = eng.infer(xd)
    assert y.dtype == BF and torch.equal(y, eager)
    (yo,) = Engine.build(net, (x,), device=device).infer(xd)
    err = T.field_err(yo, ref, 2)
    print(f"MEASURED sfno_net diagonal bf16 engine (optimized) per-field rel-L2 {err:.3e}")
    assert err < T.TOL_LAYER
