"""The bf16 precision of ``fno_mix`` and its consumers, CPU tier: the dtype rule of the op (all-bf16 operands give a
bf16 result, every other combination is mixed and returned in fp32 as before), ``fno_mix_out``, the ``fno_mix_info``
route query, the per-mode SFNO operator (``SphericalConv2d(operator="diagonal")``) and ``mix="expand"``.

Error measures (tests/test_sfno_bf16.py derives them; the GPU tier, tests/test_fno_mix_bf16_gpu.py, shares the cases):

* elementwise against the exact fp64 product of the same bf16 operands, |out - ref| <= 2^-8 |ref| + K 2^-22 S with
  S = sum_i |x| |w| over the real interleaved form and K = ceil32(2 Cin).  Products of two bf16 values are exact in
  fp32; the stream kernel's 2 Cin FMA roundings and 3 reduction adds (2^-24 relative each) and the MFMA kernel's
  accumulation over at most K terms both stay inside K 2^-22 S with a margin of 4;
* per field against the fp64 product with the unrounded fp32 weights: 1e-2 (``TOL_KERNEL``);
* layers against the fp64 torch backend, per field: 2e-2 (``TOL_LAYER``)."""
import re

import pytest
import torch

from test_sfno_bf16 import TOL_KERNEL, TOL_LAYER, assert_exact_product, ceil_to, field_err
from tensorrt_dft_plugins_amd.models import SFNOConfig, SFNONet, sfno
from tensorrt_dft_plugins_amd.models.sfno import SFNOBlock, SphericalConv2d
from tensorrt_dft_plugins_amd.onnx import exporter as ex
from tensorrt_dft_plugins_amd.onnx import proto as P
from tensorrt_dft_plugins_amd.onnx.runner import OnnxGraph
from tensorrt_dft_plugins_amd.ops import spectral as SP

BF = torch.bfloat16
ops = torch.ops.amd_dft
ids = lambda c: "x".join(map(str, c))  # noqa: E731

_CASES = {}


def fmix_case(case):
    """Of one (B, Cin, Cout, M): x bf16, the fp32 weights, their bf16 rounding, (ref, S) of the exact product of the
    bf16 operands over the real interleaved form, and the fp64 product with the unrounded weights.  Built once per
    case and left unchanged."""
    if case not in _CASES:
        B, Cin, Cout, M = case
        g = torch.Generator().manual_seed(1000 * B + 100 * Cin + 10 * Cout + M)
        x = torch.randn(B, Cin, M, 2, generator=g).to(BF)
        w = torch.randn(Cin, Cout, M, 2, generator=g) / Cin ** 0.5
        wb = w.to(BF)
        xd, wd = x.double(), wb.double()
        y = torch.view_as_real(torch.einsum("bim,iom->bom", torch.view_as_complex(xd), torch.view_as_complex(wd)))
        ar, ai, wr, wi = xd[..., 0].abs(), xd[..., 1].abs(), wd[..., 0].abs(), wd[..., 1].abs()
        S = torch.stack([torch.einsum("bim,iom->bom", ar, wr) + torch.einsum("bim,iom->bom", ai, wi),
                         torch.einsum("bim,iom->bom", ai, wr) + torch.einsum("bim,iom->bom", ar, wi)], -1)
        yu = torch.view_as_real(torch.einsum("bim,iom->bom", torch.view_as_complex(xd),
                                             torch.view_as_complex(w.double())))
        _CASES[case] = (x, w, wb, (y, S), yu)
    return _CASES[case]


def check_fmix(out, case, what):
    B, Cin, Cout, M = case
    _, _, _, exact, unrounded = fmix_case(case)
    assert out.shape == (B, Cout, M, 2) and out.dtype == BF and out.is_contiguous()
    assert_exact_product(out, *exact, ceil_to(2 * Cin, 32), f"fno_mix bf16 {what} {case}")
    err = field_err(out, unrounded, 2)
    print(f"MEASURED fno_mix bf16 {what} {case} vs unrounded weights {err:.3e}")
    assert err < TOL_KERNEL


def fields(info):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", info)}


# ------------------------------------------------------------------------------------------------ the op
CPU_CASES = [(2, 5, 7, 19), (1, 20, 20, 33), (9, 3, 2, 5)]


@pytest.mark.parametrize("case", CPU_CASES, ids=ids)
def test_fno_mix_all_bf16_returns_bf16(case):
    x, _, wb, _, _ = fmix_case(case)
    for path in (0, 2):
        check_fmix(ops.fno_mix(x, wb, path), case, f"cpu path={path}")
    check_fmix(SP.fno_spectral_mix(x, wb), case, "cpu wrapper")


@pytest.mark.parametrize("case", CPU_CASES[:2], ids=ids)
def test_fno_mix_mixed_dtypes_stay_fp32(case):
    """bf16 x with fp32 w, the reverse and all-fp32: upcast, the fp32 einsum, an fp32 result -- the formula of the op
    before it had bf16 kernels."""
    x, w, wb, _, _ = fmix_case(case)

    def formula(a, b):
        return torch.view_as_real(torch.einsum("bim,iom->bom", torch.view_as_complex(a.float().contiguous()),
                                               torch.view_as_complex(b.float().contiguous()))).contiguous()

    for a, b in ((x, w), (x.float(), wb), (x.float(), w), (x.double(), w)):
        out = ops.fno_mix(a, b, 0)
        assert out.dtype == torch.float32 and torch.equal(out, formula(a, b))


def test_fno_mix_meta():
    x = torch.empty(3, 5, 11, 2, device="meta", dtype=BF)
    w = torch.empty(5, 7, 11, 2, device="meta", dtype=BF)
    for a, b, dt in ((x, w, BF), (x.float(), w, torch.float32), (x, w.float(), torch.float32),
                     (x.float(), w.float(), torch.float32)):
        y = ops.fno_mix(a, b, 0)
        assert y.device.type == "meta" and y.shape == (3, 7, 11, 2) and y.dtype == dt
        o = torch.empty(3, 7, 11, 2, device="meta", dtype=dt)
        assert ops.fno_mix_out(a, b, 0, o) is o


def test_fno_mix_out_cpu():
    case = CPU_CASES[0]
    B, Cin, Cout, M = case
    x, w, wb, _, _ = fmix_case(case)
    o16 = torch.full((B, Cout, M, 2), float("nan"), dtype=BF)
    assert ops.fno_mix_out(x, wb, 0, o16) is o16
    assert torch.equal(o16, ops.fno_mix(x, wb, 0))
    o32 = torch.full((B, Cout, M, 2), float("nan"))
    assert ops.fno_mix_out(x.float(), w, 0, o32) is o32
    assert torch.equal(o32, ops.fno_mix(x.float(), w, 0))
    assert torch.equal(ops.fno_mix_out(x, w, 0, o32), ops.fno_mix(x, w, 0))  # a mixed call writes fp32
    with pytest.raises(RuntimeError, match="out must be"):
        ops.fno_mix_out(x, wb, 0, o32)  # an fp32 out for a bf16 call
    with pytest.raises(RuntimeError, match="out must be"):
        ops.fno_mix_out(x.float(), w, 0, o16)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.fno_mix_out(x, wb, 0, torch.empty(B, Cout, M + 1, 2, dtype=BF))
    with pytest.raises(RuntimeError, match="not contiguous"):
        ops.fno_mix_out(x, wb, 0, torch.empty(B, Cout, 2, M, dtype=BF).transpose(2, 3))
    with pytest.raises(RuntimeError, match="fno_mix: x"):
        ops.fno_mix_out(x, wb[:, :, :-1], 0, o16)


def test_fno_mix_info():
    info = ops.fno_mix_info
    # fp32: what the op has always done -- the stream kernel up to B = 8, the MFMA kernel (8 modes) above or on
    # request, the stream kernel 8 samples per launch where the fp32 tile is beyond 160 KB
    for B, nb in ((1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8)):
        s = info(B, 20, 20, 2048)
        assert s == f"stream NB={nb} vec=1 lds={3 * nb * 64 * 8} wgs=640 launches=1" and info(B, 20, 20, 2048, False, 0) == s
    s = info(9, 20, 20, 2048)
    assert s == f"mfma MT=8 lds={32 * (16 * 40 + 40 * 48 + 16 * 48)} wgs=256 launches=1"
    assert info(2, 20, 20, 2048, False, 2) == s
    assert info(32, 20, 20, 2048) == f"mfma MT=8 lds={32 * (32 * 40 + 40 * 48 + 32 * 48)} wgs=256 launches=1"
    assert info(20, 40, 40, 100) == "stream-batched NB=8 vec=1 lds=12288 wgs=63 launches=3"
    assert info(4, 40, 40, 100, False, 2) == "stream NB=4 vec=1 lds=6144 wgs=63 launches=1"  # no tile: the request is moot
    # bf16: the same switch at B = 8 | 9, the K-major tile (pitch 2 ceil32(2 Cin) + 16 bytes)
    # the stream kernel takes two modes per lane (8-byte loads) where M is even
    assert info(8, 20, 20, 2048, True) == "stream NB=8 vec=2 lds=24576 wgs=320 launches=1 bf16=1"
    assert info(1, 20, 20, 4096, True) == "stream NB=1 vec=2 lds=3072 wgs=640 launches=1 bf16=1"
    assert info(1, 20, 20, 4095, True) == "stream NB=1 vec=1 lds=1536 wgs=1280 launches=1 bf16=1"
    per_mode = (16 + 48) * 144 + 32 + 16 * 48 * 2 + 4
    assert 8 * per_mode > 80 * 1024 >= 4 * per_mode
    assert info(9, 20, 20, 2048, True) == f"mfma MT=4 lds={4 * per_mode} wgs=512 launches=1 bf16=1"
    assert info(2, 20, 20, 2048, True, 2) == info(9, 20, 20, 2048, True)
    # narrow channels: 16 modes fit 80 KB, and the tile halves while fewer than 256 workgroups would run
    per_mode = (16 + 16) * 80 + 32 + 16 * 16 * 2 + 4
    assert info(12, 4, 4, 8192, True) == f"mfma MT=16 lds={16 * per_mode} wgs=512 launches=1 bf16=1"
    assert info(12, 4, 4, 2048, True) == f"mfma MT=8 lds={8 * per_mode} wgs=256 launches=1 bf16=1"
    assert info(12, 4, 4, 37, True) == f"mfma MT=4 lds={4 * per_mode} wgs=10 launches=1 bf16=1"
    # 4 modes beyond 80 KB but within 160 KB; and beyond that: batched
    per_mode = (32 + 96) * 208 + 32 + 32 * 96 * 2 + 4
    assert 80 * 1024 < 4 * per_mode <= 160 * 1024
    assert info(32, 48, 48, 64, True) == f"mfma MT=4 lds={4 * per_mode} wgs=16 launches=1 bf16=1"
    assert info(9, 96, 96, 5, True) == "stream-batched NB=8 vec=1 lds=12288 wgs=8 launches=2 bf16=1"
    assert info(17, 72, 40, 3, True) == "stream-batched NB=8 vec=1 lds=12288 wgs=2 launches=3 bf16=1"
    assert info(10, 96, 96, 4, True) == "stream-batched NB=8 vec=2 lds=24576 wgs=3 launches=2 bf16=1"
    # bf16 tiles are smaller: width 40 has no fp32 tile and has a bf16 one
    assert info(9, 40, 40, 100).startswith("stream-batched") and info(9, 40, 40, 100, True).startswith("mfma MT=4")
    with pytest.raises(RuntimeError, match="fno_mix_info"):
        info(0, 20, 20, 64)


# ------------------------------------------------------------------------------------------------ layers
DIAG_SHAPE, DIAG_L, DIAG_M = (2, 5, 17, 32), 12, 9


def diag_refs(shape, lmax, mmax, grid="equiangular", operator="diagonal", seed=30):
    """(x bf16, a SphericalConv2d and an SFNOBlock of ``operator`` whose parameters are bf16 values held in fp32, the
    fp64 torch-backend results of both on x)."""
    _, C, nlat, nlon = shape
    torch.manual_seed(seed)
    x = torch.randn(*shape).to(BF)
    conv = SphericalConv2d(C, C, nlat, nlon, lmax, mmax, grid, backend="torch", operator=operator)
    blk = SFNOBlock(C, nlat, nlon, lmax, mmax, grid, backend="torch", operator=operator)
    with torch.no_grad():
        for p in list(conv.parameters()) + list(blk.parameters()):
            p.copy_(p.to(BF).float())
        ref_c = conv.double()(x.double())
        ref_b = blk.double()(x.double())
    return x, conv.float().set_backend("amd"), blk.float().set_backend("amd"), ref_c, ref_b


def spy_mix(monkeypatch, calls):
    """Record the dtypes of every ``fno_spectral_mix`` call; ``sfno_mix`` fails the test."""
    real = SP.fno_spectral_mix

    def spy(xm, w):
        calls.append((xm.dtype, w.dtype))
        return real(xm, w)

    monkeypatch.setattr(SP, "fno_spectral_mix", spy)
    monkeypatch.setattr(SP, "sfno_mix", lambda *a, **k: pytest.fail("the layer ran sfno_mix"))


def test_diagonal_operator_cpu(monkeypatch):
    x, conv, blk, ref_c, ref_b = diag_refs(DIAG_SHAPE, DIAG_L, DIAG_M)
    C = DIAG_SHAPE[1]
    assert conv.weight.shape == (C, C, DIAG_L, DIAG_M, 2) and conv.operator == "diagonal"
    fresh = SphericalConv2d(C, C, 17, 32, DIAG_L, DIAG_M, operator="diagonal").weight.detach()  # the dhconv scale
    assert 0.9 / (C * C) < float(fresh.max()) <= 1.0 / (C * C) and float(fresh.min()) >= 0.0
    # not the per-degree operator: the weights vary over m
    wd = conv.weight.detach()
    assert float((wd[:, :, :, 0] - wd[:, :, :, 1]).abs().max()) > 0
    calls = []
    spy_mix(monkeypatch, calls)
    with torch.no_grad():
        for dt, tol in ((torch.float32, 1e-5), (BF, TOL_LAYER)):
            out_c, out_b = conv(x.to(dt)), blk(x.to(dt))
            assert out_c.shape == x.shape and out_c.dtype == dt and out_b.dtype == dt
            e_c, e_b = field_err(out_c, ref_c, 2), field_err(out_b, ref_b, 2)
            print(f"MEASURED sfno diagonal cpu {dt} conv {e_c:.3e} block {e_b:.3e}")
            assert e_c < tol and e_b < tol
    assert calls == [(torch.float32, torch.float32)] * 2 + [(BF, BF)] * 2
    # the bf16 weights are cast once, cached, and follow the parameter
    w16 = conv._mode_weight(BF)
    assert conv._mode_weight(BF) is w16 and w16.dtype == BF and w16.shape == (C, C, DIAG_L * DIAG_M, 2)
    with torch.no_grad():
        conv.weight.mul_(2.0)
    assert conv._mode_weight(BF) is not w16
    with pytest.raises(ValueError, match="operator"):
        SphericalConv2d(2, 2, 9, 16, operator="bogus")
    with pytest.raises(ValueError, match="operator"):
        SFNONet(SFNOConfig(img_size=(9, 16), operator="bogus"))


def test_mix_expand_cpu(monkeypatch):
    """``mix="expand"``: ``fno_mix`` on the expansion in both dtypes, bf16 tensors for a bf16 input."""
    x, conv, blk, ref_c, ref_b = diag_refs(DIAG_SHAPE, DIAG_L, DIAG_M, operator="dhconv")
    conv.mix = blk.spectral.mix = "expand"
    calls = []
    spy_mix(monkeypatch, calls)
    with torch.no_grad():
        for dt, tol in ((torch.float32, 1e-5), (BF, TOL_LAYER)):
            out_c, out_b = conv(x.to(dt)), blk(x.to(dt))
            assert out_c.dtype == dt and out_b.dtype == dt
            e_c, e_b = field_err(out_c, ref_c, 2), field_err(out_b, ref_b, 2)
            print(f"MEASURED sfno expand cpu {dt} conv {e_c:.3e} block {e_b:.3e}")
            assert e_c < tol and e_b < tol
    assert calls == [(torch.float32, torch.float32)] * 2 + [(BF, BF)] * 2
    e16, e32 = conv._expanded_weight(BF), conv._expanded_weight()
    assert conv._expanded_weight(BF) is e16 and e16.dtype == BF and e32.dtype == torch.float32
    assert torch.equal(e16, e32.to(BF)) and e16.shape == (5, 5, DIAG_L * DIAG_M, 2)
    monkeypatch.setattr(sfno, "EXPAND_LIMIT_BYTES", conv.expanded_bytes() - 1)
    for dt in (torch.float32, BF):
        with pytest.raises(ValueError, match="EXPAND_LIMIT_BYTES"):
            conv(x.to(dt))
    with pytest.raises(ValueError, match="mix"):
        SphericalConv2d(2, 2, 9, 16, mix="bogus")
    assert SphericalConv2d(2, 2, 9, 16, mix="expand").mix == "expand"


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
def test_sfno_net_diagonal_export_runner(dt):
    torch.manual_seed(0)
    net = SFNONet(SFNOConfig(img_size=(17, 32), in_chans=3, out_chans=2, embed_dim=6, depth=2, lmax=8, mmax=8,
                             operator="diagonal")).eval()
    assert net.blocks[0].layer.spectral.weight.shape == (6, 6, 8, 8, 2)
    x = torch.randn(2, 3, 17, 32).to(dt)
    with torch.no_grad():
        for p in net.parameters():  # bf16 values held in fp32: the oracle sees the weights the bf16 network sees
            p.copy_(p.to(BF).float())
        eager = net(x)
        ref = net.set_backend("torch")(x.double())
        net.set_backend("amd")
    assert eager.dtype == dt
    err = field_err(eager, ref, 2)
    print(f"MEASURED sfno_net diagonal cpu {dt} per-field rel-L2 {err:.3e}")
    assert err < (1e-5 if dt == torch.float32 else TOL_LAYER)
    data = ex.export(net, (x,))
    nodes = P.load_model(data).graph.node
    compute = {n.op_type for n in nodes if n.domain == "com.amd.dft"}
    assert {"fno_pointwise", "instance_norm", "legendre", "fno_mix"} <= compute and "sfno_mix" not in compute
    (y,) = OnnxGraph(data, torch.device("cpu")).run(x)
    assert y.dtype == dt and torch.equal(y, eager)
