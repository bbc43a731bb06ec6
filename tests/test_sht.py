"""Spherical harmonic transforms, CPU tier: the quadrature / Legendre tables in fp64, analytic fields through
``sht`` / ``isht``, the ``legendre`` op (ATen kernel, Meta shapes, argument errors, ``legendre_info``) and the SFNO
modules (``backend="amd"`` on CPU tensors against ``backend="torch"``)."""
import math
import re

import numpy as np
import pytest
import torch

from tensorrt_dft_plugins_amd import isht, sht
from tensorrt_dft_plugins_amd.models import sfno
from tensorrt_dft_plugins_amd.models.sfno import InverseRealSHT, RealSHT, SFNOBlock, SphericalConv2d
from tensorrt_dft_plugins_amd.ops import spectral as SP
from tensorrt_dft_plugins_amd.ops.sht import legendre_tables
from helpers import rel_l2


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("grid", ["legendre-gauss", "equiangular"])
@pytest.mark.parametrize("nlat", [2, 12, 33, 46])
def test_weights_sum_to_two(grid, nlat):
    x, w, _ = legendre_tables(nlat, 2, 2, grid)
    assert x.dtype == np.float64 and w.dtype == np.float64
    assert abs(w.sum() - 2.0) < 1e-13
    assert np.all(np.diff(x) < 0)  # north to south
    if grid == "equiangular":
        assert abs(x[0] - 1.0) < 1e-15 and abs(x[-1] + 1.0) < 1e-15  # poles included


# Clenshaw-Curtis integrates polynomials up to degree nlat - 1 exactly, so lmax stays within l + l' <= nlat - 1
@pytest.mark.parametrize("grid,nlat,lmax", [("legendre-gauss", 12, 12), ("legendre-gauss", 45, 45), ("equiangular", 33, 16)])
def test_orthonormality(grid, nlat, lmax):
    _, w, P = legendre_tables(nlat, lmax, lmax, grid)
    assert P.shape == (lmax, lmax, nlat) and P.dtype == np.float64
    for m in range(lmax):
        G = 2.0 * np.pi * (P[m] * w) @ P[m].T
        I = np.diag((np.arange(lmax) >= m).astype(np.float64))  # Pb_l^m = 0 where l < m
        assert np.abs(G - I).max() < 1e-10, m


@pytest.mark.parametrize("grid", ["legendre-gauss", "equiangular"])
def test_m0_rows_match_numpy_legendre(grid):
    lmax = 40
    x, _, P = legendre_tables(37, lmax, 3, grid)
    for l in range(lmax):
        c = np.zeros(l + 1)
        c[l] = 1.0
        ref = math.sqrt((2 * l + 1) / (4 * math.pi)) * np.polynomial.legendre.legval(x, c)
        assert np.abs(P[0, l] - ref).max() < 1e-12, l


def test_closed_forms_with_condon_shortley_sign():
    x, _, P = legendre_tables(21, 4, 3, "legendre-gauss")
    s = np.sqrt(1.0 - x * x)
    assert abs(P[0, 0, 0] - 1.0 / math.sqrt(4 * math.pi)) < 1e-15
    assert np.abs(P[1, 1] - (-math.sqrt(3.0 / (8 * math.pi)) * s)).max() < 1e-14
    assert np.abs(P[1, 2] - (-math.sqrt(15.0 / (8 * math.pi)) * s * x)).max() < 1e-14
    assert np.abs(P[2, 2] - (math.sqrt(15.0 / (32 * math.pi)) * s * s)).max() < 1e-14
    assert np.all(P[1, 0] == 0.0) and np.all(P[2, 1] == 0.0)


def test_bad_grid_and_mmax_raise():
    with pytest.raises(ValueError):
        legendre_tables(8, 4, 4, "lobatto")
    with pytest.raises(ValueError):
        sht(torch.zeros(1, 8, 16), mmax=10)
    with pytest.raises(TypeError):
        sht(torch.zeros(1, 8, 16, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ analytic fields
def _grid(nlat, nlon, grid):
    x, _, _ = legendre_tables(nlat, 1, 1, grid)
    theta = torch.from_numpy(np.arccos(np.clip(x, -1, 1)))[:, None]
    phi = (2 * math.pi * torch.arange(nlon, dtype=torch.float64) / nlon)[None, :]
    return theta, phi


@pytest.mark.parametrize("grid", ["legendre-gauss", "equiangular"])
def test_analytic_fields_give_single_coefficients(grid):
    nlat, nlon, L = 33, 64, 12
    theta, phi = _grid(nlat, nlon, grid)
    one = torch.ones(nlat, nlon, dtype=torch.float64)
    fields = torch.stack([one, torch.cos(theta) * one, torch.sin(theta) * torch.cos(phi)]).float()
    c = sht(fields, L, L, grid)
    assert c.shape == (3, L, L, 2) and c.dtype == torch.float32
    # f = sum c_lm Y_lm with Y_00 = 1/sqrt(4 pi), Y_10 = sqrt(3/(4 pi)) cos, Y_11 = -sqrt(3/(8 pi)) sin e^{i phi};
    # sin(theta) cos(phi) = 2 Re(c_11 Y_11) gives c_11 = -sqrt(2 pi / 3)
    expect = [((0, 0), math.sqrt(4 * math.pi)), ((1, 0), math.sqrt(4 * math.pi / 3)), ((1, 1), -math.sqrt(2 * math.pi / 3))]
    for i, ((l, m), v) in enumerate(expect):
        ref = torch.zeros(L, L, 2)
        ref[l, m, 0] = v
        assert (c[i] - ref).abs().max() < 2e-6, (grid, l, m, c[i, l, m])


@pytest.mark.parametrize("grid,nlat,nlon,L", [("legendre-gauss", 24, 48, 24), ("equiangular", 33, 64, 16)])
def test_round_trip_band_limited(grid, nlat, nlon, L):
    g = torch.Generator().manual_seed(nlat)
    c = torch.randn(2, 3, L, L, 2, generator=g)
    c = c * (torch.arange(L)[:, None] >= torch.arange(L)[None, :])[:, :, None]
    c[..., 0, 1] = 0.0
    f = isht(c, nlat, nlon, grid)  # a band-limited random field
    assert f.shape == (2, 3, nlat, nlon)
    c2 = sht(f, L, L, grid)
    f2 = isht(c2, nlat, nlon, grid)
    assert rel_l2(c2, c) < 1e-5
    assert rel_l2(f2, f) < 1e-5
    assert rel_l2(isht(torch.view_as_complex(c2), nlat, nlon, grid), f) < 1e-5  # complex input


# ------------------------------------------------------------------------------------------------ ops
def _zeroed(table, tri):
    M, R, Q = table.shape
    m = torch.arange(M)[:, None]
    t = table.clone()
    if tri == 1:
        t *= (torch.arange(R)[None, :] >= m)[:, :, None]
    elif tri == 2:
        t *= (torch.arange(Q)[None, :] >= m)[:, None, :]
    return t


@pytest.mark.parametrize("tri", [0, 1, 2])
def test_legendre_cpu_vs_fp64(tri):
    g = torch.Generator().manual_seed(tri)
    N, Q, R, M = 3, 21, 13, 9
    x = torch.randn(2, N, Q, M, 2, generator=g)
    table = torch.randn(M, R, Q, generator=g) / Q ** 0.5
    ref = torch.einsum("mrq,bnqmc->bnrmc", _zeroed(table, tri).double(), x.double())
    out = torch.ops.amd_dft.legendre(x, _zeroed(table, tri), None, tri)
    assert out.shape == (2, N, R, M, 2) and out.dtype == torch.float32
    assert rel_l2(out, ref) < 1e-6
    # the part tri declares zero is treated as zero whatever it holds
    assert rel_l2(torch.ops.amd_dft.legendre(x, table, None, tri), ref) < 1e-6


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_legendre_cpu_ignores_x_where_tri2_declares_zero(poison):
    """``tri = 2``: x[n, q < m, m] is not read -- a NaN or Inf there gives the product of x with that part zeroed
    (a masked table alone would give 0 * NaN = NaN), as the GPU kernel, which stages that part as zero."""
    g = torch.Generator().manual_seed(5)
    N, Q, R, M = 3, 21, 13, 9
    x = torch.randn(N, Q, M, 2, generator=g)
    table = torch.randn(M, R, Q, generator=g) / Q ** 0.5
    below = (torch.arange(Q)[:, None] < torch.arange(M)[None, :])[None, :, :, None].expand(N, Q, M, 2)
    ref = torch.einsum("mrq,nqmc->nrmc", table.double(), torch.where(below, 0.0, x).double())
    out = torch.ops.amd_dft.legendre(torch.where(below, poison, x), table, None, 2)
    assert torch.isfinite(out).all()
    assert rel_l2(out, ref) < 1e-6


def test_legendre_cpu_out_variant():
    """A NaN-filled ``out`` equals the allocating op's result bit for bit; a wrong-shape or non-contiguous ``out``
    is an error, never a copy."""
    op, op_out = torch.ops.amd_dft.legendre, torch.ops.amd_dft.legendre_out
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, 21, 9, 2, generator=g)
    table = torch.randn(9, 13, 21, generator=g)
    for tri in (0, 1, 2):
        ref = op(x, table, None, tri)
        out = torch.full_like(ref, float("nan"))
        assert op_out(x, table, None, tri, out) is out
        assert torch.equal(out, ref)
    with pytest.raises(RuntimeError, match="out must be"):
        op_out(x, table, None, 0, torch.empty(2, 3, 13, 8, 2))
    with pytest.raises(RuntimeError, match="out must be"):
        op_out(x, table, None, 0, torch.empty(2, 3, 13, 9, 4)[..., ::2])
    with pytest.raises(RuntimeError, match="out must be"):
        op_out(x, table, None, 0, torch.empty(2, 3, 13, 9, 2, dtype=torch.float64))
    m = op_out(x.to("meta"), table.to("meta"), None, 0, torch.empty(2, 3, 13, 9, 2, device="meta"))
    assert m.device.type == "meta" and m.shape == (2, 3, 13, 9, 2)


def test_legendre_meta_shapes():
    x = torch.empty(2, 5, 45, 13, 2, device="meta")
    t = torch.empty(13, 23, 45, device="meta")
    y = torch.ops.amd_dft.legendre(x, t, None, 1)
    assert y.device.type == "meta" and y.shape == (2, 5, 23, 13, 2) and y.dtype == torch.float32
    assert torch.ops.amd_dft.legendre(x[0, 0], t, None, 0).shape == (23, 13, 2)


def test_legendre_argument_errors():
    op = torch.ops.amd_dft.legendre
    x, t = torch.zeros(2, 8, 4, 2), torch.zeros(4, 6, 8)
    assert op(x, t, None, 0).shape == (2, 6, 4, 2)
    with pytest.raises(RuntimeError, match="transformed dim"):
        op(torch.zeros(2, 7, 4, 2), t, None, 0)
    with pytest.raises(RuntimeError, match="mode counts"):
        op(torch.zeros(2, 8, 5, 2), t, None, 0)
    with pytest.raises(RuntimeError, match="float32"):
        op(x.to(torch.bfloat16), t, None, 0)
    with pytest.raises(RuntimeError, match="float32"):
        op(x, t.double(), None, 0)
    with pytest.raises(RuntimeError, match="tri"):
        op(x, t, None, 3)
    with pytest.raises(RuntimeError, match="table_split"):
        op(x, t, torch.zeros(2, 4, 6, 8, dtype=torch.bfloat16), 0)  # not padded to [2, 4, 16, 32]
    with pytest.raises(RuntimeError):
        op(torch.zeros(8, 4), t, None, 0)


def _fields(s):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", s)}


def test_legendre_info_routes():
    info = torch.ops.amd_dft.legendre_info
    # (Q, R, M, cols) -> (MT, CT): a full grid keeps the 8-mode x 16-field tile; fewer workgroups than CUs drop to
    # 4 modes, then to 8 fields; M <= 4 and cols <= 16 have nothing to fill the larger tile with
    for (Q, R, M, cols), (mt, ct) in {(40, 200, 80, 256): (8, 2), (40, 100, 80, 256): (4, 2), (90, 90, 46, 80): (4, 1),
                                      (720, 64, 64, 40): (4, 1), (32, 16, 8, 4): (4, 1), (64, 4096, 4, 4096): (4, 2),
                                      (64, 64, 4096, 16): (8, 1), (45, 23, 13, 6): (4, 1)}.items():
        for tri in (0, 1, 2):
            s = info(Q, R, M, cols, tri)
            f = _fields(s)
            assert s.startswith("mfma ") and (f["MT"], f["CT"]) == (mt, ct), s
            assert f["slabs"] == -(-Q // 32) and f["rtiles"] == -(-R // 16) and f["rgroups"] == -(-f["rtiles"] // 4), s
            assert f["mgroups"] == -(-M // mt) and f["ctiles"] == -(-cols // (16 * ct)), s
            assert f["wgs"] == f["mgroups"] * f["ctiles"] * f["rgroups"] and f["tri"] == tri, s
            xs = 2 * mt * (16 * ct * 80 + 256 // mt)
            ys = 16 * (8 * ct * (2 * mt + 2) + 4) * 4
            assert f["lds"] == max(xs, ys) and 2 * f["lds"] <= 160 * 1024, s
    for bad in ((0, 4, 4, 4, 0), (4, 0, 4, 4, 0), (4, 4, 0, 4, 0), (4, 4, 4, 3, 0), (4, 4, 4, 4, 3)):
        with pytest.raises(RuntimeError):
            info(*bad)


# ------------------------------------------------------------------------------------------------ modules
@pytest.mark.parametrize("grid,nlat,nlon,lmax,mmax", [("equiangular", 17, 32, None, None), ("legendre-gauss", 12, 24, 10, 7)])
def test_sht_modules_amd_equals_torch_on_cpu(grid, nlat, nlon, lmax, mmax):
    g = torch.Generator().manual_seed(nlon)
    x = torch.randn(2, 3, nlat, nlon, generator=g)
    fa, ft = RealSHT(nlat, nlon, lmax, mmax, grid), RealSHT(nlat, nlon, lmax, mmax, grid, backend="torch")
    assert fa.backend == "amd" and (fa.lmax, fa.mmax) == ((nlat, min(nlat, nlon // 2 + 1)) if lmax is None else (lmax, mmax))
    ca, ct = fa(x), ft(x)
    assert ca.is_complex() and ca.shape == (2, 3, fa.lmax, fa.mmax) and ct.shape == ca.shape
    assert rel_l2(ca, ct) < 1e-6
    ia = InverseRealSHT(nlat, nlon, fa.lmax, fa.mmax, grid)
    it = InverseRealSHT(nlat, nlon, fa.lmax, fa.mmax, grid, backend="torch")
    ya, yt = ia(ct), it(ct)
    assert ya.shape == x.shape and not ya.is_complex()
    assert rel_l2(ya, yt) < 1e-6
    assert rel_l2(ft(x.double()), ct) < 1e-6 and ft(x.double()).dtype == torch.complex128  # the fp64 oracle
    with pytest.raises(ValueError):
        fa(x[..., :-1])
    with pytest.raises(ValueError):
        RealSHT(nlat, nlon, backend="cuda")


def _conv_definition(conv, x):
    """isht(sum_i sht(x)[b,i,l,m] w[i,o,l]) with the torch-backend transforms in fp64."""
    s = conv.sht
    fwd = RealSHT(s.nlat, s.nlon, s.lmax, s.mmax, s.grid, backend="torch")
    inv = InverseRealSHT(s.nlat, s.nlon, s.lmax, s.mmax, s.grid, backend="torch")
    w = torch.view_as_complex(conv.weight.detach().double().contiguous())
    return inv(torch.einsum("bilm,iol->bolm", fwd(x.double()), w))


def test_spherical_conv_equals_definition():
    torch.manual_seed(5)
    conv = SphericalConv2d(5, 7, 17, 32, 12, 9)
    assert conv.weight.shape == (5, 7, 12, 2)
    x = torch.randn(2, 5, 17, 32)
    ref = _conv_definition(conv, x)
    with torch.no_grad():
        ya = conv(x)
        yt = conv.set_backend("torch")(x)
    assert ya.shape == (2, 7, 17, 32)
    assert rel_l2(ya, ref) < 1e-6 and rel_l2(yt, ref) < 1e-6


def test_spherical_conv_expansion_is_cached_and_follows_the_weights():
    torch.manual_seed(6)
    conv = SphericalConv2d(3, 3, 9, 16)
    x = torch.randn(1, 3, 9, 16)
    with torch.no_grad():
        conv(x)
        w0 = conv._expanded_weight()
        assert conv._expanded_weight() is w0 and w0.shape == (3, 3, conv.sht.lmax * conv.sht.mmax, 2)
        conv.weight.mul_(2.0)
        assert conv._expanded_weight() is not w0
        assert rel_l2(conv(x), _conv_definition(conv, x)) < 1e-6


def test_spherical_conv_fallback_above_the_expansion_bound(monkeypatch):
    """With the bound patched to zero the layer must not expand its weights: it notes a ``sfno_mix`` fallback (counted
    on GPU tensors, an error under strict mode) and mixes with einsum -- same result."""
    torch.manual_seed(7)
    conv = SphericalConv2d(4, 4, 9, 16)
    x = torch.randn(1, 4, 9, 16)
    assert conv.expanded_bytes() == 4 * 4 * 9 * 9 * 2 * 4 <= sfno.EXPAND_LIMIT_BYTES == 256 << 20
    notes = []
    monkeypatch.setattr(SP, "note_fallback", lambda op, why, t: notes.append(op))
    monkeypatch.setattr(SP, "fno_spectral_mix", lambda *a: pytest.fail("expanded weights used above the bound"))
    monkeypatch.setattr(sfno, "EXPAND_LIMIT_BYTES", 0)
    with torch.no_grad():
        y = conv(x)
    assert notes == ["sfno_mix"]
    assert rel_l2(y, _conv_definition(conv, x)) < 1e-6


def test_sfno_block_amd_equals_torch_on_cpu():
    torch.manual_seed(8)
    blk = SFNOBlock(6, 17, 32, 8, 8)
    x = torch.randn(2, 6, 17, 32)
    with torch.no_grad():
        ya = blk(x)
        yt = blk.set_backend("torch")(x)
        ref = torch.nn.functional.gelu(_conv_definition(blk.spectral, x) + blk.w.double()(x.double()))
    assert rel_l2(ya, ref) < 1e-6 and rel_l2(yt, ref) < 1e-6
    blk.float()
    lin = SFNOBlock(6, 17, 32, 8, 8, activation=False)
    with torch.no_grad():
        assert rel_l2(lin(x), lin.set_backend("torch")(x)) < 1e-6
