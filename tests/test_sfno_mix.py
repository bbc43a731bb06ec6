"""SFNO per-degree channel mixing, CPU tier: the ``sfno_mix`` op (ATen kernel, Meta shapes, argument errors), the
weight table of ``sfno_mix_split``, the tiling ``sfno_mix_info`` reports, and the SFNO layers with ``mix="degree"``
on CPU tensors against the fp64 definition."""
import re

import pytest
import torch

from tensorrt_dft_plugins_amd.models import sfno
from tensorrt_dft_plugins_amd.models.sfno import InverseRealSHT, RealSHT, SFNOBlock, SphericalConv2d
from tensorrt_dft_plugins_amd.ops import spectral as SP
from helpers import rel_l2


def _mix_ref(c, w, tri):
    """fp64 complex einsum of the same fp32 inputs; ``tri = 1``: zero where l < m."""
    y = torch.einsum("bilm,iol->bolm", torch.view_as_complex(c.double()), torch.view_as_complex(w.double()))
    if tri:
        L, M = c.shape[2], c.shape[3]
        y = y * (torch.arange(L)[:, None] >= torch.arange(M)[None, :])
    return torch.view_as_real(y)


def _below(B, Cout, L, M):
    return (torch.arange(L)[:, None] < torch.arange(M)[None, :])[None, None, :, :, None].expand(B, Cout, L, M, 2)


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("case", [(2, 5, 7, 12, 9), (1, 3, 2, 4, 11)], ids=lambda c: "x".join(map(str, c)))
def test_sfno_mix_cpu_vs_fp64(case, tri):
    """Random input everywhere, also where l < m: ``tri = 1`` ignores it there and returns exact zeros."""
    B, Cin, Cout, L, M = case
    g = torch.Generator().manual_seed(sum(case))
    c, w = torch.randn(B, Cin, L, M, 2, generator=g), torch.randn(Cin, Cout, L, 2, generator=g)
    y = SP.sfno_mix(c, w, tri=tri)
    assert y.shape == (B, Cout, L, M, 2) and y.dtype == torch.float32 and y.is_contiguous()
    assert rel_l2(y, _mix_ref(c, w, tri)) < 1e-6
    assert rel_l2(SP.sfno_mix(c, w, SP.sfno_mix_split(w), tri), _mix_ref(c, w, tri)) < 1e-6
    if tri:
        assert torch.all(y[_below(B, Cout, L, M)] == 0.0)
    else:
        assert rel_l2(y, _mix_ref(c, w, 1)) > 1e-2  # the orders above l were used


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_sfno_mix_cpu_ignores_c_where_l_below_m(poison):
    """``tri = 1``: c[b, i, l, m > l] is not read -- a NaN or Inf there gives the product of the zeroed spectrum, with
    exact 0.0 where l < m."""
    B, Cin, Cout, L, M = 2, 5, 7, 12, 9
    g = torch.Generator().manual_seed(7)
    c, w = torch.randn(B, Cin, L, M, 2, generator=g), torch.randn(Cin, Cout, L, 2, generator=g)
    y = SP.sfno_mix(torch.where(_below(B, Cin, L, M), poison, c), w, tri=1)
    assert torch.isfinite(y).all()
    assert rel_l2(y, _mix_ref(c, w, 1)) < 1e-6
    assert torch.all(y[_below(B, Cout, L, M)] == 0.0)


def test_sfno_mix_cpu_out_variant():
    """A NaN-filled ``out`` equals the allocating op's result bit for bit; a wrong-shape or non-contiguous ``out``
    is an error, never a copy."""
    op, op_out = torch.ops.amd_dft.sfno_mix, torch.ops.amd_dft.sfno_mix_out
    g = torch.Generator().manual_seed(8)
    c, w = torch.randn(2, 5, 12, 9, 2, generator=g), torch.randn(5, 7, 12, 2, generator=g)
    for tri in (0, 1):
        ref = op(c, w, None, tri)
        out = torch.full_like(ref, float("nan"))
        assert op_out(c, w, None, tri, out) is out
        assert torch.equal(out, ref)
    with pytest.raises(RuntimeError, match="out must be"):
        op_out(c, w, None, 0, torch.empty(2, 5, 12, 9, 2))
    with pytest.raises(RuntimeError, match="out must be"):
        op_out(c, w, None, 0, torch.empty(2, 7, 12, 9, 4)[..., ::2])
    m = op_out(c.to("meta"), w.to("meta"), None, 0, torch.empty(2, 7, 12, 9, 2, device="meta"))
    assert m.device.type == "meta" and m.shape == (2, 7, 12, 9, 2)


def test_sfno_mix_meta():
    c = torch.empty(3, 5, 12, 9, 2, device="meta")
    w = torch.empty(5, 7, 12, 2, device="meta")
    y = torch.ops.amd_dft.sfno_mix(c, w, None, 1)
    assert y.shape == (3, 7, 12, 9, 2) and y.dtype == torch.float32 and y.device.type == "meta"


def test_sfno_mix_argument_errors():
    op = torch.ops.amd_dft.sfno_mix
    c, w = torch.zeros(2, 5, 6, 4, 2), torch.zeros(5, 7, 6, 2)
    assert op(c, w, None, 0).shape == (2, 7, 6, 4, 2)
    with pytest.raises(RuntimeError, match="float32"):
        op(c.to(torch.bfloat16), w, None, 0)
    with pytest.raises(RuntimeError, match="float32"):
        op(c, w.double(), None, 0)
    with pytest.raises(RuntimeError, match=r"c \[B, Cin, L, M, 2\]"):
        op(c[0], w, None, 0)
    with pytest.raises(RuntimeError, match=r"c \[B, Cin, L, M, 2\]"):
        op(c, w[..., 0], None, 0)
    with pytest.raises(RuntimeError, match="input channels"):
        op(torch.zeros(2, 4, 6, 4, 2), w, None, 0)
    with pytest.raises(RuntimeError, match="degree counts"):
        op(torch.zeros(2, 5, 7, 4, 2), w, None, 0)
    with pytest.raises(RuntimeError, match="tri"):
        op(c, w, None, 2)
    with pytest.raises(RuntimeError, match="w_split"):
        op(c, w, torch.zeros(2, 6, 7, 10, dtype=torch.bfloat16), 0)  # not padded to [2, 6, 16, 32]
    with pytest.raises(RuntimeError, match="w_split"):
        op(c, w, torch.zeros(2, 6, 16, 32), 0)  # not bfloat16
    with pytest.raises(RuntimeError, match="float32"):
        torch.ops.amd_dft.sfno_mix_split(w.double())
    with pytest.raises(RuntimeError):
        torch.ops.amd_dft.sfno_mix_split(torch.zeros(5, 7, 6))


# ------------------------------------------------------------------------------------------------ the weight table
@pytest.mark.parametrize("shape", [(5, 7, 6), (16, 16, 3), (17, 33, 2)], ids=lambda s: "x".join(map(str, s)))
def test_sfno_mix_split_table(shape):
    Cin, Cout, L = shape
    g = torch.Generator().manual_seed(Cin + Cout)
    w = torch.randn(Cin, Cout, L, 2, generator=g)
    ts = SP.sfno_mix_split(w)
    Op, Kp = (Cout + 15) // 16 * 16, (2 * Cin + 31) // 32 * 32
    assert ts.shape == (2, L, Op, Kp) and ts.dtype == torch.bfloat16 and ts.is_contiguous()
    both = ts.float().sum(0)  # hi + lo, exact in fp32
    live = both[:, :Cout, :2 * Cin].reshape(L, Cout, Cin, 2)
    want = w.permute(2, 1, 0, 3)  # [L, Cout, Cin, (Wr | Wi)]: k = 2 i -> Wr, k = 2 i + 1 -> Wi
    assert torch.all((live - want).abs() <= 2.0 ** -16 * want.abs())
    assert torch.equal(ts[0, :, :Cout, :2 * Cin], want.reshape(L, Cout, 2 * Cin).to(torch.bfloat16))  # hi = bf16(w)
    pad = torch.ones(Op, Kp, dtype=torch.bool)
    pad[:Cout, :2 * Cin] = False
    assert torch.all(ts.float()[:, :, pad] == 0.0)


# ------------------------------------------------------------------------------------------------ the tiling
def _fields(s):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", s)}


def test_sfno_mix_info():
    info = torch.ops.amd_dft.sfno_mix_info
    for B, Cin, Cout, L, M in [(1, 3, 5, 7, 5), (2, 20, 20, 23, 13), (3, 32, 64, 16, 16), (1, 40, 72, 9, 33),
                               (5, 16, 16, 70, 70), (2, 130, 24, 12, 12), (1, 256, 256, 180, 180)]:
        f0, f1 = _fields(info(B, Cin, Cout, L, M, 0)), _fields(info(B, Cin, Cout, L, M, 1))
        for tri, f in ((0, f0), (1, f1)):
            assert f["slabs"] == (2 * Cin + 31) // 32 and f["otiles"] == (Cout + 15) // 16
            assert f["ogroups"] == (f["otiles"] + 3) // 4 and f["coltile"] == 64 and f["tri"] == tri
            assert f["lds"] == 2 * 128 * 80 <= 80 * 1024
            assert f["wgs"] <= f["grid"] == f["ctiles"] * f["ogroups"] * L
        # workgroups that multiply: per degree ceil(B Ml / 64) column tiles, Ml = M or min(M, l + 1)
        assert f0["wgs"] == L * ((B * M + 63) // 64) * f0["ogroups"] == f0["grid"]
        assert f1["wgs"] == sum((B * min(M, l + 1) + 63) // 64 for l in range(L)) * f1["ogroups"]
        assert f1["wgs"] <= f0["wgs"]
    assert _fields(info(1, 64, 64, 180, 180, 1))["wgs"] < _fields(info(1, 64, 64, 180, 180, 0))["wgs"]
    for bad in ((0, 4, 4, 4, 4, 0), (4, 0, 4, 4, 4, 0), (4, 4, 0, 4, 4, 0), (4, 4, 4, 0, 4, 0), (4, 4, 4, 4, 0, 0),
                (4, 4, 4, 4, 4, 2)):
        with pytest.raises(RuntimeError):
            info(*bad)


# ------------------------------------------------------------------------------------------------ the layers
def _conv_definition(conv, x):
    """isht(sum_i sht(x)[b,i,l,m] w[i,o,l]) with the torch-backend transforms in fp64."""
    s = conv.sht
    fwd = RealSHT(s.nlat, s.nlon, s.lmax, s.mmax, s.grid, backend="torch")
    inv = InverseRealSHT(s.nlat, s.nlon, s.lmax, s.mmax, s.grid, backend="torch")
    w = torch.view_as_complex(conv.weight.detach().double().contiguous())
    return inv(torch.einsum("bilm,iol->bolm", fwd(x.double()), w))


def test_spherical_conv_degree_equals_definition(monkeypatch):
    torch.manual_seed(5)
    conv = SphericalConv2d(5, 7, 17, 32, 12, 9, mix="degree")
    monkeypatch.setattr(conv, "_expanded_weight", lambda: pytest.fail("mix='degree' built the expansion"))
    monkeypatch.setattr(SP, "fno_spectral_mix", lambda *a: pytest.fail("mix='degree' ran fno_mix"))
    x = torch.randn(2, 5, 17, 32)
    with torch.no_grad():
        y = conv(x)
    assert y.shape == (2, 7, 17, 32) and y.dtype == torch.float32
    assert rel_l2(y, _conv_definition(conv, x)) < 1e-6
    # the table is cached on the module and follows the weights
    t0 = conv._degree_weight()
    assert conv._degree_weight() is t0 and t0.shape == (2, 12, 16, 32)
    with torch.no_grad():
        conv.weight.mul_(2.0)
        y2 = conv(x)
    assert conv._degree_weight() is not t0
    assert rel_l2(y2, 2.0 * y) < 1e-6


def test_spherical_conv_auto_keeps_the_expanded_route_below_the_bound(monkeypatch):
    torch.manual_seed(6)
    conv = SphericalConv2d(4, 4, 9, 16)
    assert conv.mix == "auto"
    monkeypatch.setattr(SP, "sfno_mix", lambda *a, **k: pytest.fail("per-degree op used below the bound"))
    x = torch.randn(1, 4, 9, 16)
    with torch.no_grad():
        assert rel_l2(conv(x), _conv_definition(conv, x)) < 1e-6


def test_sfno_block_degree_equals_torch_backend():
    torch.manual_seed(8)
    blk = SFNOBlock(6, 17, 32, 8, 8, mix="degree")
    assert blk.spectral.mix == "degree"
    x = torch.randn(2, 6, 17, 32)
    with torch.no_grad():
        ya = blk(x)
        yt = blk.set_backend("torch")(x)
        ref = torch.nn.functional.gelu(_conv_definition(blk.spectral, x) + blk.w.double()(x.double()))
    assert rel_l2(ya, yt) < 1e-6
    assert rel_l2(ya, ref) < 1e-6


def test_bad_mix_raises():
    with pytest.raises(ValueError, match="mix"):
        SphericalConv2d(4, 4, 9, 16, mix="bogus")
    with pytest.raises(ValueError, match="mix"):
        SFNOBlock(4, 9, 16, mix="bogus")
    assert sfno.EXPAND_LIMIT_BYTES == 256 << 20
