"""Vector spherical harmonic transforms on CPU tensors: the derivative tables, the fp64 ``"torch"`` backend of
``RealVectorSHT`` / ``InverseRealVectorSHT`` (the definition), the ``legendre_vec`` op's ATen kernel, ``vsht`` /
``ivsht`` and their ONNX export.  The hand kernel under them: tests/test_vsht_gpu.py, which shares the references
built here.

Conventions and formulas: ``tensorrt_dft_plugins_amd/ops/sht.py``.  Round trips stay where the quadrature is exact
for the products involved: ``legendre-gauss`` up to lmax = nlat, ``equiangular`` up to lmax = (nlat + 1) / 2."""
import math
import re

import numpy as np
import pytest
import torch

import tensorrt_dft_plugins_amd as tdp
from tensorrt_dft_plugins_amd.engine import Engine
from tensorrt_dft_plugins_amd.models.sfno import InverseRealSHT, InverseRealVectorSHT, RealSHT, RealVectorSHT
from tensorrt_dft_plugins_amd.onnx import exporter as ex
from tensorrt_dft_plugins_amd.onnx import proto as P
from tensorrt_dft_plugins_amd.onnx.runner import OnnxGraph
from tensorrt_dft_plugins_amd.ops import sht as S

BF = torch.bfloat16
ops = torch.ops.amd_dft
TOL = 1e-5        # fp32, per field: the bound of tests/test_sht_gpu.py
TOL_BF16 = 2e-2   # bf16 transforms, per field: the project's bound (tests/test_sfno_bf16.py)
# (grid, nlat, nlon, lmax, mmax): where vsht(ivsht(c)) = c
GRIDS = [("legendre-gauss", 24, 48, 24, 13), ("legendre-gauss", 33, 64, 20, 9), ("equiangular", 25, 48, 13, 13),
         ("equiangular", 24, 48, 12, 12)]
gid = lambda g: f"{g[0]}-{g[1]}-{g[3]}-{g[4]}"  # noqa: E731


def fields(info):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", info)}


def field_err(out, ref, lead):
    """max over the ``lead`` leading dims (fields, or fields x components) of the rel-L2 against the fp64 reference"""
    o = out.detach().cpu()
    if o.is_complex():
        o = torch.view_as_real(o.to(torch.complex128))
    if ref.is_complex():
        ref = torch.view_as_real(ref)
    o = o.double()
    n = math.prod(o.shape[:lead])
    o, r = o.reshape(n, -1), ref.reshape(n, -1)
    num, den = (o - r).norm(dim=1), r.norm(dim=1)
    return float(torch.where(den > 0, num / den, num).max())


def coefficients(lead, lmax, mmax, seed):
    """Random fp64 coefficients [*lead, 2, lmax, mmax, 2] of a real vector field: supported on l >= max(m, 1), real at
    m = 0."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(*lead, 2, lmax, mmax, 2, generator=g, dtype=torch.float64)
    keep = torch.arange(lmax)[:, None] >= torch.arange(mmax).clamp(min=1)[None, :]
    c = c * keep[:, :, None]
    c[..., 0, 1] = 0.0
    return c


# ------------------------------------------------------------------------------------------------ tables
def _pbar(theta, lmax, mmax):
    """Pb_l^m(cos theta) [mmax, lmax, len(theta)] at any colatitudes, by the recurrence of ``legendre_tables``."""
    x, s = np.cos(theta), np.sin(theta)
    Pb = np.zeros((mmax, lmax, len(theta)))
    pmm = np.full(len(theta), 1.0 / math.sqrt(4.0 * math.pi))
    for m in range(min(mmax, lmax)):
        if m > 0:
            pmm = -math.sqrt((2.0 * m + 1.0) / (2.0 * m)) * s * pmm
        Pb[m, m] = pmm
        for l in range(m + 1, lmax):
            a = math.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
            b = math.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0)) if l > m + 1 else 0.0
            Pb[m, l] = a * (x * Pb[m, l - 1] - (b * Pb[m, l - 2] if l > m + 1 else 0.0))
    return Pb


@pytest.mark.parametrize("grid", S.GRIDS)
def test_vector_table_identities(grid):
    nlat, lmax, mmax = 24, 12, 12
    x, w, D0, D1 = S.vector_legendre_tables(nlat, lmax, mmax, grid)
    x2, w2, Pb = S.legendre_tables(nlat, lmax, mmax, grid)
    assert np.array_equal(x, x2) and np.array_equal(w, w2)
    assert D0.shape == D1.shape == (mmax, lmax, nlat) and D0.dtype == D1.dtype == np.float64
    theta = np.arccos(x)
    assert np.abs(_pbar(theta, lmax, mmax) - Pb).max() < 1e-13  # the helper is the library's recurrence
    live = (np.arange(lmax)[None, :] >= np.maximum(np.arange(mmax), 1)[:, None])[:, :, None]
    h = 1e-6
    diff = (_pbar(theta + h, lmax, mmax) - _pbar(theta - h, lmax, mmax)) / (2 * h)
    e0 = np.abs(D0 - diff * live).max()
    m = np.arange(mmax)[:, None, None]
    e1 = np.abs(D1 * np.sin(theta) - m * Pb * live)[:, :, 1:-1].max()
    print(f"MEASURED vector tables {grid}: D0 vs central difference {e0:.3e}, D1 sin - m Pb {e1:.3e}")
    assert e0 < 1e-7
    assert e1 < 1e-12
    assert np.isfinite(D0).all() and np.isfinite(D1).all()  # the equiangular grid has both poles
    if grid == "equiangular":
        assert abs(np.sin(theta[0])) < 1e-15 and np.abs(D1[1, :, 0]).max() > 0.1  # m = 1 survives at the pole
    assert not (D0 * ~live).any() and not (D1 * ~live).any() and not D1[0].any()
    assert np.abs(D0[:, :, 1:-1]).max(axis=2)[live[:, :, 0]].min() > 0.1  # and no live row is


def test_vsht_tables_cache_per_dtype():
    t32 = S.vsht_tables(9, 16, 9, 9, "equiangular", "cpu")
    t16 = S.vsht_tables(9, 16, 9, 9, "equiangular", "cpu", BF)
    assert S.vsht_tables(9, 16, 9, 9, "equiangular", "cpu", torch.float32) is t32
    assert S.vsht_tables(9, 16, 9, 9, "equiangular", "cpu", BF) is t16 and t16 is not t32
    assert S.sht_tables(9, 16, 9, 9, "equiangular", "cpu") is not t32  # the vector tag keeps the keys apart
    for n in t32.NAMES:
        assert getattr(t32, n).dtype == torch.float32 and torch.equal(getattr(t16, n), getattr(t32, n).to(BF))
        assert getattr(t32, n + "_split") is None  # split forms on a GPU only
    assert t32.fwd_a.shape == (9, 9, 9) and not t32.fwd_a[:, 0].any() and not t32.fwd_b[0].any()
    with pytest.raises(TypeError):
        S.vsht_tables(9, 16, 9, 9, "equiangular", "cpu", torch.float64)


# ------------------------------------------------------------------------------------------------ the definition
_PAIR = {}


def pair(g):
    """(forward, inverse) torch-backend modules of one grid, built once."""
    if g not in _PAIR:
        grid, nlat, nlon, lmax, mmax = g
        _PAIR[g] = (RealVectorSHT(nlat, nlon, lmax, mmax, grid, backend="torch"),
                    InverseRealVectorSHT(nlat, nlon, lmax, mmax, grid, backend="torch"))
    return _PAIR[g]


@pytest.mark.parametrize("g", GRIDS, ids=gid)
def test_round_trip_fp64(g):
    grid, nlat, nlon, lmax, mmax = g
    fwd, inv = pair(g)
    c = torch.view_as_complex(coefficients((3,), lmax, mmax, nlat))
    v = inv(c)
    assert v.shape == (3, 2, nlat, nlon) and v.dtype == torch.float64
    c2 = fwd(v)
    assert c2.shape == c.shape and c2.dtype == torch.complex128
    err = float((c2 - c).norm() / c.norm())
    print(f"MEASURED vsht(ivsht(c)) fp64 {g} rel-L2 {err:.3e}")
    assert err < 1e-12


@pytest.mark.parametrize("g", GRIDS, ids=gid)
def test_gradient_is_spheroidal_fp64(g):
    """v = grad f for a band-limited scalar f: s = sht(f) for l >= 1, t = 0."""
    grid, nlat, nlon, lmax, mmax = g
    fwd, _ = pair(g)
    cf = coefficients((2,), lmax, mmax, 7 + nlat)[:, 0]  # [2, lmax, mmax, 2]
    cf = torch.view_as_complex(cf.contiguous())
    f = InverseRealSHT(nlat, nlon, lmax, mmax, grid, backend="torch")(cf)
    _, _, D0, D1 = S.vector_legendre_tables(nlat, lmax, mmax, grid)
    # d f / d theta = sum_l D0 c; (1 / sin theta) d f / d phi = sum_l (i m Pb / sin theta) c = i sum_l D1 c
    u = torch.einsum("mlk,nlm->nkm", torch.from_numpy(D0).to(torch.complex128), cf)
    w = 1j * torch.einsum("mlk,nlm->nkm", torch.from_numpy(D1).to(torch.complex128), cf)
    v = torch.fft.irfft(torch.stack([u, w], dim=1), n=nlon, dim=-1, norm="forward")
    st = fwd(v)
    s, t = st[:, 0], st[:, 1]
    sf = RealSHT(nlat, nlon, lmax, mmax, grid, backend="torch")(f)
    e_s = float((s[:, 1:] - sf[:, 1:]).norm() / sf[:, 1:].norm())
    e_t = float(t.norm() / s.norm())
    print(f"MEASURED gradient identity {g}: |s - sht(f)| / |sht(f)| {e_s:.3e}, |t| / |s| {e_t:.3e}")
    assert not s[:, 0].abs().max() > 0
    assert e_s < 1e-12
    assert e_t < 1e-12


# ------------------------------------------------------------------------------------------------ the op
# (N, Q, R, M) of legendre_vec: x [N, 2, Q, M, 2], tables [M, R, Q].  The three grids of the GPU tier in the forward
# direction -- (nlat 33, lmax 20, mmax 9) x 3 fields: a ragged second slab, a ragged row tile, M % 4 != 0, an odd
# field count | (25, 13, 13) x 17: past one workgroup's fields | (70, 70, 21) x 2: three slabs, two row groups
OP_CASES = [(3, 33, 20, 9), (17, 25, 13, 13), (2, 70, 70, 21)]
ids = lambda c: "x".join(map(str, c))  # noqa: E731


def zeroed(table, tri):
    """The table with the part that ``tri`` declares zero set to zero."""
    M, R, Q = table.shape
    m = torch.arange(M)[:, None]
    if tri == 1:
        return table * (torch.arange(R)[None, :] >= m)[:, :, None]
    if tri == 2:
        return table * (torch.arange(Q)[None, :] >= m)[:, None, :]
    return table


def vec_product(ta, tb, x):
    """The definition in fp64: y0 = A x0 - i B x1, y1 = A x1 + i B x0 -> real [N, 2, R, M, 2]."""
    xc = torch.view_as_complex(x.double().contiguous())
    a = torch.einsum("mrq,ncqm->ncrm", ta.double().to(torch.complex128), xc)
    b = torch.einsum("mrq,ncqm->ncrm", tb.double().to(torch.complex128), xc)
    return torch.view_as_real(torch.stack([a[:, 0] - 1j * b[:, 1], a[:, 1] + 1j * b[:, 0]], dim=1))


def vec_abs_sum(ta, tb, x):
    """sum |a| |x0| + sum |b| |x1| of every output element (component 1: x1 and x0), the re/im each term reads."""
    xa = x.double().abs()
    a = torch.einsum("mrq,ncqmp->ncrmp", ta.double().abs(), xa)
    b = torch.einsum("mrq,ncqmp->ncrmp", tb.double().abs(), xa).flip(-1)  # B's operand is the other part: re <-> im
    return a + b.flip(1)


_CASE = {}


def op_case(case, bf16=False):
    """Of one (N, Q, R, M): x, two dense random tables (all rounded to bf16 if ``bf16``) and per tri the fp64 product
    of these very operands with the declared-zero part of the tables zero, and its sum of magnitudes."""
    key = (case, bf16)
    if key not in _CASE:
        N, Q, R, M = case
        g = torch.Generator().manual_seed(N * 1000 + Q + R + M)
        x = torch.randn(N, 2, Q, M, 2, generator=g)
        ta = torch.randn(M, R, Q, generator=g) / Q ** 0.5
        tb = torch.randn(M, R, Q, generator=g) / Q ** 0.5
        if bf16:
            x, ta, tb = x.to(BF), ta.to(BF), tb.to(BF)
        refs, sums = {}, {}
        for tri in (0, 1, 2):
            refs[tri] = vec_product(zeroed(ta, tri), zeroed(tb, tri), x)
            if bf16:
                sums[tri] = vec_abs_sum(zeroed(ta, tri), zeroed(tb, tri), x)
        _CASE[key] = (x, ta, tb, refs, sums)
    return _CASE[key]


def assert_bf16_product(out, ref, asum, Q, what):
    """|out - ref| <= 2^-8 |ref| + K 2^-22 S, K = 2 ceil32(Q), for every element: the model of
    tests/test_sfno_bf16.py (one rounding of the result, fp32 accumulation over the padded length), with both tables'
    terms in S."""
    o = out.detach().cpu().double()
    assert o.shape == ref.shape and torch.isfinite(o).all(), what
    bound = 2.0 ** -8 * ref.abs() + 2 * (-(-Q // 32) * 32) * 2.0 ** -22 * asum
    diff = (o - ref).abs()
    ratio = float(torch.where(bound > 0, diff / bound, diff * float("inf")).nan_to_num(0.0, posinf=float("inf")).max())
    print(f"MEASURED {what} worst |out - ref| / bound {ratio:.3f}")
    assert torch.all(diff <= bound), what


def below_rows(N, R, M):
    return (torch.arange(R)[:, None] < torch.arange(M)[None, :])[None, None, :, :, None].expand(N, 2, R, M, 2)


def below_cols(N, Q, M):
    return (torch.arange(Q)[:, None] < torch.arange(M)[None, :])[None, None, :, :, None].expand(N, 2, Q, M, 2)


@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case", OP_CASES, ids=ids)
def test_legendre_vec_cpu(case, tri):
    N, Q, R, M = case
    x, ta, tb, refs, _ = op_case(case)
    out = ops.legendre_vec(x, ta, tb, None, None, tri)
    assert out.shape == (N, 2, R, M, 2) and out.dtype == torch.float32 and out.is_contiguous()
    err = field_err(out, refs[tri], 2)
    print(f"MEASURED legendre_vec cpu {case} tri={tri} {err:.3e}")
    assert err < TOL
    if tri == 0:
        assert field_err(out, refs[1], 2) > 1e-2 and field_err(out, refs[2], 2) > 1e-2
    if tri == 1:
        assert torch.all(out[below_rows(N, R, M)] == 0.0)
    o2 = torch.full((N, 2, R, M, 2), float("nan"))
    assert ops.legendre_vec_out(x, ta, tb, None, None, tri, o2) is o2
    assert torch.equal(o2, out)
    # leading dims are kept
    assert torch.equal(ops.legendre_vec(x.unsqueeze(0), ta, tb, None, None, tri), out.unsqueeze(0))


def test_legendre_vec_cpu_bf16():
    case = OP_CASES[0]
    x, ta, tb, refs, sums = op_case(case, True)
    for tri in (0, 1, 2):
        out = ops.legendre_vec(x, ta, tb, None, None, tri)
        assert out.dtype == BF
        assert_bf16_product(out, refs[tri], sums[tri], case[1], f"legendre_vec cpu bf16 tri={tri}")


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_legendre_vec_cpu_ignores_x_where_tri2_declares_zero(poison):
    case = OP_CASES[1]
    N, Q, R, M = case
    x, ta, tb, refs, _ = op_case(case)
    out = ops.legendre_vec(torch.where(below_cols(N, Q, M), poison, x), ta, tb, None, None, 2)
    assert torch.isfinite(out).all()
    assert field_err(out, refs[2], 2) < TOL


def test_legendre_vec_errors_and_meta():
    N, Q, R, M = OP_CASES[0]
    x, ta, tb, _, _ = op_case(OP_CASES[0])
    with pytest.raises(RuntimeError, match="must all be float32 or all be bfloat16"):
        ops.legendre_vec(x, ta, tb.to(BF))
    with pytest.raises(RuntimeError, match="must all be float32 or all be bfloat16"):
        ops.legendre_vec(x.to(BF), ta, tb)
    with pytest.raises(RuntimeError, match="must all be float32 or all be bfloat16"):
        ops.legendre_vec(x.double(), ta.double(), tb.double())
    with pytest.raises(RuntimeError, match=r"x \[\.\.\., 2, Q, M, 2\]"):
        ops.legendre_vec(x[:, 0], ta, tb)  # no component dim (N = 3 is not 2)
    with pytest.raises(RuntimeError, match="same shape"):
        ops.legendre_vec(x, ta, tb[:, :-1])
    with pytest.raises(RuntimeError, match="points along the transformed dim"):
        ops.legendre_vec(x[:, :, :-1], ta, tb)
    with pytest.raises(RuntimeError, match="mode counts differ"):
        ops.legendre_vec(x[:, :, :, :-1], ta, tb)
    with pytest.raises(RuntimeError, match="tri must be"):
        ops.legendre_vec(x, ta, tb, None, None, 3)
    with pytest.raises(RuntimeError, match="ta_split and tb_split must be bfloat16"):
        ops.legendre_vec(x, ta, tb, torch.zeros(2, M, R, Q, dtype=BF), None, 0)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.legendre_vec_out(x, ta, tb, None, None, 0, torch.empty(N, 2, R, M + 1, 2))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.legendre_vec_out(x, ta, tb, None, None, 0, torch.empty(N, 2, R, M, 2, dtype=BF))
    for dt in (torch.float32, BF):
        xm, am, bm = (t.to(dt).to("meta") for t in (x, ta, tb))
        ym = ops.legendre_vec(xm.unsqueeze(0), am, bm, None, None, 1)
        assert ym.shape == (1, N, 2, R, M, 2) and ym.dtype == dt and ym.device.type == "meta"
        om = torch.empty(N, 2, R, M, 2, dtype=dt, device="meta")
        assert ops.legendre_vec_out(xm, am, bm, None, None, 1, om) is om


def test_legendre_vec_info():
    s = ops.legendre_vec_info(33, 20, 9, 12, 1)
    f = fields(s)
    assert s.startswith("mfma ") and "bf16" not in f
    assert (f["MT"], f["CT"], f["slabs"], f["rtiles"], f["rgroups"], f["mgroups"], f["ctiles"], f["tri"]) == \
        (4, 1, 2, 2, 1, 3, 1, 1)
    assert f["wgs"] == f["rgroups"] * f["mgroups"] * f["ctiles"] and f["lds"] == 10752
    fb = fields(ops.legendre_vec_info(33, 20, 9, 12, 1, True))
    assert fb["bf16"] == 1 and fb["lds"] == 5376
    # fp32 never takes 8 modes per workgroup; bf16 does once the grid fills the device
    assert fields(ops.legendre_vec_info(33, 200, 252, 36, 0))["MT"] == 4
    assert fields(ops.legendre_vec_info(33, 200, 252, 36, 0, True))["MT"] == 8
    for bad in ((0, 4, 4, 4, 0), (4, 4, 4, 6, 0), (4, 4, 4, 4, 3)):
        with pytest.raises(RuntimeError, match="legendre_vec_info"):
            ops.legendre_vec_info(*bad)


# ------------------------------------------------------------------------------------------------ transforms
_TR = {}


def transform_case(g, lead):
    """Of one grid: a band-limited field v (fp32-rounded, from random coefficients), random fp32 coefficients c, and
    the fp64 torch backend's vsht(v) and ivsht(c) on those very inputs."""
    key = (g, lead)
    if key not in _TR:
        grid, nlat, nlon, lmax, mmax = g
        fwd, inv = pair(g)
        v = inv(torch.view_as_complex(coefficients(lead, lmax, mmax, 3 * nlat))).float()
        c = coefficients(lead, lmax, mmax, 5 * nlat).float()
        if nlon % 2 == 0 and mmax == nlon // 2 + 1:
            c[..., -1, 1] = 0.0  # a real field's Nyquist mode is real too
        _TR[key] = (v, c, fwd(v.double()), inv(torch.view_as_complex(c.double())))
    return _TR[key]


@pytest.mark.parametrize("g", GRIDS, ids=gid)
def test_vsht_ivsht_cpu_vs_fp64(g):
    grid, nlat, nlon, lmax, mmax = g
    v, c, ref_f, ref_i = transform_case(g, (2, 3))
    out = tdp.vsht(v, lmax, mmax, grid)
    assert out.shape == (2, 3, 2, lmax, mmax, 2) and out.dtype == torch.float32
    e_f = field_err(torch.view_as_complex(out), ref_f, 2)
    out_i = tdp.ivsht(c, nlat, nlon, grid)
    assert out_i.shape == (2, 3, 2, nlat, nlon) and out_i.dtype == torch.float32
    e_i = field_err(out_i, ref_i, 2)
    assert torch.equal(tdp.ivsht(torch.view_as_complex(c), nlat, nlon, grid), out_i)  # complex64 is accepted
    mf = RealVectorSHT(nlat, nlon, lmax, mmax, grid).to(v.device)
    mi = InverseRealVectorSHT(nlat, nlon, lmax, mmax, grid).to(v.device)
    assert mf.backend == "amd" and torch.equal(torch.view_as_real(mf(v)), out)
    assert torch.equal(mi(torch.view_as_complex(c)), out_i)
    print(f"MEASURED vsht cpu {g} fwd {e_f:.3e} inv {e_i:.3e}")
    assert e_f < TOL
    assert e_i < TOL
    # bf16 in and out, against the same transforms of the bf16 inputs in fp64
    fwd, inv = pair(g)
    ob = tdp.vsht(v.to(BF), lmax, mmax, grid)
    oib = tdp.ivsht(c.to(BF), nlat, nlon, grid)
    assert ob.dtype == BF and oib.dtype == BF
    e_fb = field_err(ob, torch.view_as_real(fwd(v.to(BF).double())), 2)
    e_ib = field_err(oib, inv(torch.view_as_complex(c.to(BF).double())), 2)
    print(f"MEASURED vsht cpu bf16 {g} fwd {e_fb:.3e} inv {e_ib:.3e}")
    assert e_fb < TOL_BF16
    assert e_ib < TOL_BF16


def test_vsht_defaults_and_errors():
    v = torch.randn(1, 2, 9, 16)
    assert tdp.vsht(v).shape == (1, 2, 9, 9, 2)  # lmax = nlat, mmax = min(lmax, nlon // 2 + 1)
    assert tdp.vsht(v, grid="legendre-gauss", mmax=5).shape == (1, 2, 9, 5, 2)
    with pytest.raises(TypeError):
        tdp.vsht(v.double())
    with pytest.raises(TypeError):
        tdp.ivsht(torch.zeros(1, 2, 9, 9, 2, dtype=torch.float64), 9, 16)
    with pytest.raises(ValueError):
        tdp.vsht(torch.randn(1, 3, 9, 16))
    with pytest.raises(ValueError):
        tdp.ivsht(torch.zeros(3, 9, 9, 2), 9, 16)
    with pytest.raises(ValueError):
        tdp.vsht(v, grid="healpix")
    with pytest.raises(TypeError, match=r"vsht\(\)"):
        RealVectorSHT(9, 16)(v.to(BF))
    with pytest.raises(TypeError, match=r"ivsht\(\)"):
        InverseRealVectorSHT(9, 16)(torch.zeros(1, 2, 9, 9, 2, dtype=BF))
    with pytest.raises(ValueError):
        RealVectorSHT(9, 16)(torch.randn(1, 2, 9, 18))
    with pytest.raises(ValueError):
        InverseRealVectorSHT(9, 16, backend="hip")
    assert "nlat=9" in repr(RealVectorSHT(9, 16))


# ------------------------------------------------------------------------------------------------ ONNX
class RoundTrip(torch.nn.Module):
    def __init__(self, g):
        super().__init__()
        self.grid, self.nlat, self.nlon, self.lmax, self.mmax = g

    def forward(self, x):
        return tdp.ivsht(tdp.vsht(x, self.lmax, self.mmax, self.grid), self.nlat, self.nlon, self.grid)


def test_vsht_onnx_runner_engine(tmp_path):
    g = GRIDS[2]
    net = RoundTrip(g).eval()
    v, _, _, _ = transform_case(g, (2, 3))
    with torch.no_grad():
        eager = net(v)
    assert field_err(eager, v.double(), 2) < TOL  # the field is band-limited: the round trip returns it
    data = ex.export(net, (v,))
    nodes = P.load_model(data).graph.node
    compute = [n.op_type for n in nodes if n.domain == "com.amd.dft"]
    assert compute == ["r2c", "legendre_vec", "legendre_vec", "c2r"], compute
    assert not {n.op_type for n in nodes if n.domain != "com.amd.dft"} & {"MatMul", "Einsum", "Gemm", "DFT"}
    (y,) = OnnxGraph(data, torch.device("cpu")).run(v)
    assert torch.equal(y, eager)
    eng = Engine.build(net, (v,), device="cpu")
    (ye,) = eng.infer(v)
    assert torch.equal(ye, eager)
    p = str(tmp_path / "vsht.engine")
    eng.save(p)
    (yl,) = Engine.load(p, device="cpu").infer(v)
    assert torch.equal(yl, eager)
