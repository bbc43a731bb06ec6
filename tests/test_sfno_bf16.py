"""The bf16 precision of the spherical line, CPU tier: ``legendre`` / ``sfno_mix`` (and their ``_out`` forms) on
all-bf16 operands (ATen kernels, Meta shapes, argument errors), the one-plane split tables, the ``*_info`` queries
with ``bf16=True``, and ``sht`` / ``isht`` on bf16 CPU tensors.

Two error measures, shared with the GPU tier (tests/test_sfno_bf16_gpu.py):

* elementwise against the exact product of the same bf16 operands (``assert_exact_product``).  Products of two bf16
  values are exact in fp32, so an implementation's only errors are the fp32 accumulation and the one rounding of the
  result to bf16:  |out - ref| <= 2^-8 |ref| + K 2^-22 S  with ref = sum t x and S = sum |t| |x| in fp64 and K the
  padded contraction length (ceil32(Q); ceil32(2 Cin) over the real interleaved form of ``sfno_mix``).  2^-8 covers
  the bf16 rounding, K 2^-24 S is the any-order fp32 summation bound, and the factor 4 covers the MFMA's internal
  order and rounding mode.  The bound is derived, not measured; a missing term is about S / K, far above it.
* per field (max rel-L2 over fields) against the fp64 product with the unrounded fp32 table or weights: 1e-2, the
  project's bound for one bf16-operand kernel with a bf16 store (tests/test_fno.py); a transform or a layer (several
  such kernels in a row): 2e-2, the project's bf16 layer bound."""
import re

import pytest
import torch

from tensorrt_dft_plugins_amd import isht, sht
from tensorrt_dft_plugins_amd.models import sfno
from tensorrt_dft_plugins_amd.models.sfno import InverseRealSHT, RealSHT, SFNOBlock, SphericalConv2d
from tensorrt_dft_plugins_amd.ops import spectral as SP
from tensorrt_dft_plugins_amd.ops.sht import legendre_split, sht_tables

BF = torch.bfloat16
TOL_KERNEL = 1e-2
TOL_LAYER = 2e-2
ops = torch.ops.amd_dft


def ceil_to(n, k):
    return -(-n // k) * k


def field_err(out, ref, lead):
    """max over the ``lead`` leading (field) dims of the field's rel-L2 against the fp64 reference."""
    o = out.detach().cpu().double()
    n = 1
    for d in o.shape[:lead]:
        n *= d
    o, r = o.reshape(n, -1), ref.reshape(n, -1)
    num, den = (o - r).norm(dim=1), r.norm(dim=1)
    return float(torch.where(den > 0, num / den, num).max())


def assert_exact_product(out, ref, S, K, what):
    """|out - ref| <= 2^-8 |ref| + K 2^-22 S for every element (module docstring); prints the worst ratio first."""
    o = out.detach().cpu().double()
    assert o.shape == ref.shape and torch.isfinite(o).all(), what
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -22 * S
    diff = (o - ref).abs()
    ratio = float(torch.where(bound > 0, diff / bound, diff * float("inf")).nan_to_num(0.0, posinf=float("inf")).max())
    print(f"MEASURED {what} worst |out - ref| / bound {ratio:.3f}")
    assert torch.all(diff <= bound), what


def zeroed(table, tri):
    """The table with the part that ``tri`` declares zero set to zero."""
    M, R, Q = table.shape
    m = torch.arange(M)[:, None]
    t = table.clone()
    if tri == 1:
        t = t * (torch.arange(R)[None, :] >= m)[:, :, None]
    elif tri == 2:
        t = t * (torch.arange(Q)[None, :] >= m)[:, None, :]
    return t


def keep(L, M):
    return (torch.arange(L)[:, None] >= torch.arange(M)[None, :])[:, :, None]


_LEG = {}


def legendre_case(case):
    """Of one (N, Q, R, M): x bf16, the dense random fp32 table, its bf16 rounding, and per tri (ref, S) of the exact
    product of the bf16 operands and the fp64 product with the unrounded table, the declared-zero part zero in both."""
    if case not in _LEG:
        N, Q, R, M = case
        g = torch.Generator().manual_seed(N * 1000 + Q + R + M)
        x = torch.randn(N, Q, M, 2, generator=g).to(BF)
        table = torch.randn(M, R, Q, generator=g) / Q ** 0.5
        tb = table.to(BF)
        exact, unrounded = {}, {}
        for tri in (0, 1, 2):
            t = zeroed(tb, tri).double()
            exact[tri] = (torch.einsum("mrq,nqmc->nrmc", t, x.double()),
                          torch.einsum("mrq,nqmc->nrmc", t.abs(), x.double().abs()))
            unrounded[tri] = torch.einsum("mrq,nqmc->nrmc", zeroed(table, tri).double(), x.double())
        _LEG[case] = (x, table, tb, exact, unrounded)
    return _LEG[case]


_MIX = {}


def mix_case(case):
    """Of one (B, Cin, Cout, L, M): c bf16 (random everywhere), the fp32 weights, their bf16 rounding, and per tri
    (ref, S) over the real interleaved form (K = 2 Cin: Wr against (re, im), Wi against (-im, re)) and the fp64 product
    with the unrounded weights; ``tri = 1``: c taken as zero where l < m."""
    if case not in _MIX:
        B, Cin, Cout, L, M = case
        g = torch.Generator().manual_seed(sum(case))
        c = torch.randn(B, Cin, L, M, 2, generator=g).to(BF)
        w = torch.randn(Cin, Cout, L, 2, generator=g) / Cin ** 0.5
        wb = w.to(BF)
        cd, wd = c.double(), wb.double()
        y = torch.view_as_real(torch.einsum("bilm,iol->bolm", torch.view_as_complex(cd), torch.view_as_complex(wd)))
        # S: both parts sum |Wr| |.| + |Wi| |.| over i with the roles of re and im exchanged
        ar, ai, wr, wi = cd[..., 0].abs(), cd[..., 1].abs(), wd[..., 0].abs(), wd[..., 1].abs()
        S = torch.stack([torch.einsum("bilm,iol->bolm", ar, wr) + torch.einsum("bilm,iol->bolm", ai, wi),
                         torch.einsum("bilm,iol->bolm", ai, wr) + torch.einsum("bilm,iol->bolm", ar, wi)], -1)
        yu = torch.view_as_real(torch.einsum("bilm,iol->bolm", torch.view_as_complex(cd),
                                             torch.view_as_complex(w.double())))
        k = keep(L, M)
        _MIX[case] = (c, w, wb, {0: (y, S), 1: (y * k, S * k)}, {0: yu, 1: yu * k})
    return _MIX[case]


# ------------------------------------------------------------------------------------------------ legendre
LEG_CPU = [(3, 45, 23, 13), (2, 32, 16, 8)]


@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case", LEG_CPU, ids=lambda c: "x".join(map(str, c)))
def test_legendre_bf16_cpu(case, tri):
    """All-bf16 ``legendre`` / ``legendre_out`` on CPU tensors: bf16 out, the dirty table's declared-zero part
    ignored (exact zeros in rows r < m under ``tri = 1``), with and without the one-plane split."""
    N, Q, R, M = case
    x, table, tb, exact, unrounded = legendre_case(case)
    ref, S = exact[tri]
    for ts in (None, legendre_split(tb)):
        out = ops.legendre(x, tb, ts, tri)
        assert out.shape == (N, R, M, 2) and out.dtype == BF and out.is_contiguous()
        assert_exact_product(out, ref, S, ceil_to(Q, 32), f"legendre cpu {case} tri={tri}")
        assert field_err(out, unrounded[tri], 1) < TOL_KERNEL
    if tri == 0 and M > 1:
        assert field_err(out, unrounded[1], 1) > 1e-1 and field_err(out, unrounded[2], 1) > 1e-1  # nothing skipped
    if tri == 1:
        below = (torch.arange(R)[:, None] < torch.arange(M)[None, :])[None, :, :, None].expand(N, R, M, 2)
        assert torch.all(out[below] == 0.0)
    o2 = torch.full((N, R, M, 2), float("nan"), dtype=BF)
    assert ops.legendre_out(x, tb, None, tri, o2) is o2
    assert torch.equal(o2, out)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.legendre_out(x, tb, None, tri, torch.empty(N, R, M, 2))  # an fp32 out for a bf16 call


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_legendre_bf16_cpu_ignores_x_where_tri2_declares_zero(poison):
    case = LEG_CPU[0]
    N, Q, R, M = case
    x, table, tb, exact, _ = legendre_case(case)
    below = (torch.arange(Q)[:, None] < torch.arange(M)[None, :])[None, :, :, None].expand(N, Q, M, 2)
    out = ops.legendre(torch.where(below, poison, x.float()).to(BF), tb, None, 2)
    assert_exact_product(out, *exact[2], ceil_to(Q, 32), f"legendre cpu poison {poison}")


def test_legendre_bf16_meta_and_errors():
    x = torch.empty(2, 5, 45, 13, 2, device="meta", dtype=BF)
    t = torch.empty(13, 23, 45, device="meta", dtype=BF)
    y = ops.legendre(x, t, None, 1)
    assert y.device.type == "meta" and y.shape == (2, 5, 23, 13, 2) and y.dtype == BF
    x, t = torch.zeros(2, 8, 4, 2), torch.zeros(4, 6, 8)
    for op in (lambda *a: ops.legendre(*a), lambda *a: ops.legendre_out(*a, torch.empty(2, 6, 4, 2))):
        with pytest.raises(RuntimeError, match="float32"):
            op(x.to(BF), t, None, 0)
        with pytest.raises(RuntimeError, match="float32"):
            op(x, t.to(BF), None, 0)
        with pytest.raises(RuntimeError, match="float32"):
            op(x.double(), t.double(), None, 0)
    xb, tb = x.to(BF), t.to(BF)
    assert ops.legendre(xb, tb, torch.zeros(1, 4, 16, 32, dtype=BF), 0).dtype == BF
    with pytest.raises(RuntimeError, match="table_split"):
        ops.legendre(xb, tb, torch.zeros(2, 4, 16, 32, dtype=BF), 0)  # two planes: the fp32 form
    with pytest.raises(RuntimeError, match="table_split"):
        ops.legendre(xb, tb, torch.zeros(1, 4, 6, 8, dtype=BF), 0)  # not padded
    with pytest.raises(RuntimeError, match="table_split"):
        ops.legendre(x, t, torch.zeros(1, 4, 16, 32, dtype=BF), 0)  # one plane: the bf16 form


def test_legendre_split_bf16_is_the_padded_table():
    g = torch.Generator().manual_seed(3)
    table = torch.randn(5, 23, 45, generator=g)
    ts = legendre_split(table.to(BF))
    assert ts.shape == (1, 5, 32, 64) and ts.dtype == BF and ts.is_contiguous()
    assert torch.equal(ts[0, :, :23, :45], table.to(BF))
    pad = torch.ones(32, 64, dtype=torch.bool)
    pad[:23, :45] = False
    assert torch.all(ts[0].float()[:, pad] == 0.0)
    # the one plane is the hi plane of the fp32 table's split
    assert torch.equal(ts[0], legendre_split(table)[0])


def _fields(s):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", s)}


def test_legendre_info_bf16():
    info = ops.legendre_info
    for Q, R, M, cols in [(40, 200, 80, 256), (40, 100, 80, 256), (90, 90, 46, 80), (64, 64, 4096, 16), (45, 23, 13, 6)]:
        for tri in (0, 1, 2):
            s32, s16 = info(Q, R, M, cols, tri), info(Q, R, M, cols, tri, True)
            assert info(Q, R, M, cols, tri, False) == s32 and "bf16" not in s32
            f32, f16 = _fields(s32), _fields(s16)
            assert f16.pop("bf16") == 1 and s16.endswith(" bf16=1")
            lds32, lds16 = f32.pop("lds"), f16.pop("lds")
            assert f16 == f32  # the same tiling and grid
            mt, ct = f32["MT"], f32["CT"]
            assert lds16 == max(mt * (16 * ct * 80 + 256 // mt), 16 * (8 * ct * (2 * mt + 2) + 4) * 4) < lds32


# ------------------------------------------------------------------------------------------------ sfno_mix
MIX_CPU = [(2, 5, 7, 12, 9), (1, 3, 2, 4, 11), (1, 20, 20, 9, 5)]


@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("case", MIX_CPU, ids=lambda c: "x".join(map(str, c)))
def test_sfno_mix_bf16_cpu(case, tri):
    B, Cin, Cout, L, M = case
    c, w, wb, exact, unrounded = mix_case(case)
    ref, S = exact[tri]
    for ws in (None, SP.sfno_mix_split(wb)):
        out = SP.sfno_mix(c, wb, ws, tri)
        assert out.shape == (B, Cout, L, M, 2) and out.dtype == BF and out.is_contiguous()
        assert_exact_product(out, ref, S, ceil_to(2 * Cin, 32), f"sfno_mix cpu {case} tri={tri}")
        assert field_err(out, unrounded[tri], 2) < TOL_KERNEL
    if tri:
        assert torch.all(out[(~keep(L, M))[None, None].expand(B, Cout, L, M, 2)] == 0.0)
    elif M > 1:
        assert field_err(out, unrounded[1], 2) > 1e-1  # the orders above l were used
    o2 = torch.full((B, Cout, L, M, 2), float("nan"), dtype=BF)
    assert ops.sfno_mix_out(c, wb, None, tri, o2) is o2
    assert torch.equal(o2, out)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.sfno_mix_out(c, wb, None, tri, torch.empty(B, Cout, L, M, 2))


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_sfno_mix_bf16_cpu_ignores_c_where_l_below_m(poison):
    case = MIX_CPU[0]
    B, Cin, Cout, L, M = case
    c, w, wb, exact, _ = mix_case(case)
    k = keep(L, M)[None, None].expand(B, Cin, L, M, 2)
    out = SP.sfno_mix(torch.where(k, c.float(), poison).to(BF), wb, None, 1)
    assert_exact_product(out, *exact[1], ceil_to(2 * Cin, 32), f"sfno_mix cpu poison {poison}")
    assert torch.all(out[(~keep(L, M))[None, None].expand(B, Cout, L, M, 2)] == 0.0)


def test_sfno_mix_bf16_meta_and_errors():
    c = torch.empty(3, 5, 12, 9, 2, device="meta", dtype=BF)
    w = torch.empty(5, 7, 12, 2, device="meta", dtype=BF)
    y = ops.sfno_mix(c, w, None, 1)
    assert y.shape == (3, 7, 12, 9, 2) and y.dtype == BF and y.device.type == "meta"
    c, w = torch.zeros(2, 5, 6, 4, 2), torch.zeros(5, 7, 6, 2)
    for op in (lambda *a: ops.sfno_mix(*a), lambda *a: ops.sfno_mix_out(*a, torch.empty(2, 7, 6, 4, 2))):
        with pytest.raises(RuntimeError, match="float32"):
            op(c.to(BF), w, None, 0)
        with pytest.raises(RuntimeError, match="float32"):
            op(c, w.to(BF), None, 0)
        with pytest.raises(RuntimeError, match="float32"):
            op(c.double(), w.double(), None, 0)
    cb, wb = c.to(BF), w.to(BF)
    assert ops.sfno_mix(cb, wb, torch.zeros(1, 6, 16, 32, dtype=BF), 0).dtype == BF
    with pytest.raises(RuntimeError, match="w_split"):
        ops.sfno_mix(cb, wb, torch.zeros(2, 6, 16, 32, dtype=BF), 0)  # two planes: the fp32 form
    with pytest.raises(RuntimeError, match="w_split"):
        ops.sfno_mix(cb, wb, torch.zeros(1, 6, 7, 10, dtype=BF), 0)  # not padded
    with pytest.raises(RuntimeError, match="w_split"):
        ops.sfno_mix(c, w, torch.zeros(1, 6, 16, 32, dtype=BF), 0)  # one plane: the bf16 form
    with pytest.raises(RuntimeError, match="float32"):
        ops.sfno_mix_split(w.double())


@pytest.mark.parametrize("shape", [(5, 7, 6), (16, 16, 3), (17, 33, 2)], ids=lambda s: "x".join(map(str, s)))
def test_sfno_mix_split_bf16_table(shape):
    Cin, Cout, L = shape
    g = torch.Generator().manual_seed(Cin + Cout)
    w = torch.randn(Cin, Cout, L, 2, generator=g)
    ts = SP.sfno_mix_split(w.to(BF))
    Op, Kp = ceil_to(Cout, 16), ceil_to(2 * Cin, 32)
    assert ts.shape == (1, L, Op, Kp) and ts.dtype == BF and ts.is_contiguous()
    want = w.permute(2, 1, 0, 3).reshape(L, Cout, 2 * Cin).to(BF)  # k = 2 i -> Wr, k = 2 i + 1 -> Wi
    assert torch.equal(ts[0, :, :Cout, :2 * Cin], want)
    pad = torch.ones(Op, Kp, dtype=torch.bool)
    pad[:Cout, :2 * Cin] = False
    assert torch.all(ts[0].float()[:, pad] == 0.0)
    assert torch.equal(ts[0], SP.sfno_mix_split(w)[0])  # the hi plane of the fp32 weights' split


def test_sfno_mix_info_bf16():
    info = ops.sfno_mix_info
    for B, Cin, Cout, L, M in [(1, 3, 5, 7, 5), (2, 20, 20, 23, 13), (1, 40, 72, 9, 33), (1, 256, 256, 180, 180)]:
        for tri in (0, 1):
            s32, s16 = info(B, Cin, Cout, L, M, tri), info(B, Cin, Cout, L, M, tri, True)
            assert info(B, Cin, Cout, L, M, tri, False) == s32 and "bf16" not in s32
            f32, f16 = _fields(s32), _fields(s16)
            assert f16.pop("bf16") == 1 and s16.endswith(" bf16=1")
            assert (f32.pop("lds"), f16.pop("lds")) == (2 * 128 * 80, 128 * 80)
            assert f16 == f32


# ------------------------------------------------------------------------------------------------ transforms, layers
# (shape, lmax, mmax, grid): the GPU tier's two shapes
SHT_CASES = [((2, 5, 33, 64), None, None, "equiangular"), ((1, 20, 45, 90), 23, 13, "legendre-gauss")]
SHT_IDS = ["equi33x64", "gauss45x90_l23_m13"]


def sht_refs(shape, lmax, mmax, grid):
    """(x bf16, fp64 torch-backend coefficients of x, random triangular bf16 spectrum c, its fp64 inverse)."""
    nlat, nlon = shape[-2:]
    g = torch.Generator().manual_seed(nlat)
    x = torch.randn(*shape, generator=g).to(BF)
    fwd = RealSHT(nlat, nlon, lmax, mmax, grid, backend="torch")
    inv = InverseRealSHT(nlat, nlon, fwd.lmax, fwd.mmax, grid, backend="torch")
    ref = torch.view_as_real(fwd(x.double()))
    c = torch.randn(*shape[:2], fwd.lmax, fwd.mmax, 2, generator=g)
    c = c * keep(fwd.lmax, fwd.mmax)
    c[..., 0, 1] = 0.0  # real at m = 0
    c = c.to(BF)
    return x, ref, c, inv(torch.view_as_complex(c.double())), (fwd.lmax, fwd.mmax)


@pytest.mark.parametrize("shape,lmax,mmax,grid", SHT_CASES, ids=SHT_IDS)
def test_sht_isht_bf16_cpu(shape, lmax, mmax, grid):
    nlat, nlon = shape[-2:]
    x, ref, c, ref_i, (L, M) = sht_refs(shape, lmax, mmax, grid)
    out = sht(x, lmax, mmax, grid)
    assert out.shape == (*shape[:2], L, M, 2) and out.dtype == BF
    assert torch.all(out[(~keep(L, M)).expand(*shape[:2], L, M, 2)] == 0.0)
    out_i = isht(c, nlat, nlon, grid)
    assert out_i.shape == shape and out_i.dtype == BF
    e_f, e_i = field_err(out, ref, 2), field_err(out_i, ref_i, 2)
    print(f"MEASURED sht bf16 cpu {shape} {grid} fwd {e_f:.3e} inv {e_i:.3e}")
    assert e_f < TOL_LAYER and e_i < TOL_LAYER


def test_sht_tables_cache_per_dtype():
    t32 = sht_tables(9, 16, 9, 9, "equiangular", "cpu")
    t16 = sht_tables(9, 16, 9, 9, "equiangular", "cpu", BF)
    assert sht_tables(9, 16, 9, 9, "equiangular", "cpu", torch.float32) is t32
    assert sht_tables(9, 16, 9, 9, "equiangular", "cpu", BF) is t16 and t16 is not t32
    assert t32.fwd.dtype == torch.float32 and torch.equal(t16.fwd, t32.fwd.to(BF)) and torch.equal(t16.inv, t32.inv.to(BF))
    with pytest.raises(TypeError):
        sht_tables(9, 16, 9, 9, "equiangular", "cpu", torch.float64)


def test_other_dtypes_still_raise():
    with pytest.raises(TypeError):
        sht(torch.zeros(1, 8, 16, dtype=torch.float64))
    with pytest.raises(TypeError):
        isht(torch.zeros(1, 8, 8, 2, dtype=torch.float64), 8, 16)
    with pytest.raises(TypeError):
        sht(torch.zeros(1, 8, 16, dtype=torch.float16))
    with pytest.raises(TypeError, match=r"sht\(\)"):
        RealSHT(8, 16)(torch.zeros(1, 8, 16, dtype=BF))
    with pytest.raises(TypeError, match=r"isht\(\)"):
        InverseRealSHT(8, 16)(torch.zeros(1, 8, 8, 2, dtype=BF))


MIX_CALLS = []


def pin_bf16_mix(monkeypatch, convs):
    """Which op a layer's mix runs: ``fno_mix`` and the expansion fail the test, and every ``sfno_mix`` call records
    the dtypes of (c, w, w_split) in ``MIX_CALLS`` (the layers look both ops up in ``ops.spectral`` per call)."""
    del MIX_CALLS[:]
    real = SP.sfno_mix

    def spy(c, w, w_split=None, tri=0):
        MIX_CALLS.append((c.dtype, w.dtype, w_split.dtype))
        assert tri == 1 and w_split.shape[0] == (1 if c.dtype == BF else 2)
        return real(c, w, w_split, tri)

    monkeypatch.setattr(SP, "sfno_mix", spy)
    monkeypatch.setattr(SP, "fno_spectral_mix", lambda *a: pytest.fail("a bf16 layer ran fno_mix"))
    for conv in convs:
        monkeypatch.setattr(conv, "_expanded_weight", lambda: pytest.fail("a bf16 layer built the expansion"))


def layer_refs(shape, lmax, mmax, grid, seed=20):
    """(x bf16, a SphericalConv2d and an SFNOBlock whose parameters are bf16 values held in fp32, the fp64 torch-backend
    results of both on x)."""
    _, C, nlat, nlon = shape
    torch.manual_seed(seed)
    x = torch.randn(*shape).to(BF)
    conv = SphericalConv2d(C, C, nlat, nlon, lmax, mmax, grid, backend="torch")
    blk = SFNOBlock(C, nlat, nlon, lmax, mmax, grid, backend="torch")
    with torch.no_grad():
        for p in list(conv.parameters()) + list(blk.parameters()):
            p.copy_(p.to(BF).float())
        ref_c = conv.double()(x.double())
        ref_b = blk.double()(x.double())
    return x, conv.float().set_backend("amd"), blk.float().set_backend("amd"), ref_c, ref_b


@pytest.mark.parametrize("shape,lmax,mmax,grid", SHT_CASES, ids=SHT_IDS)
def test_layers_bf16_cpu(shape, lmax, mmax, grid, monkeypatch):
    """A bf16 input runs the layers in bf16 on CPU tensors too (the ops' ATen kernels), under both ``mix`` values --
    and under both the mix is ``sfno_mix`` on bf16 tensors: ``fno_mix`` has no bf16 kernel, so the bf16 ``"auto"``
    must not take it (nor build the expansion), although the expansion is far below the limit here."""
    x, conv, blk, ref_c, ref_b = layer_refs(shape, lmax, mmax, grid)
    assert conv.expanded_bytes() < sfno.EXPAND_LIMIT_BYTES
    pin_bf16_mix(monkeypatch, [conv, blk.spectral])
    with torch.no_grad():
        for mix in ("auto", "degree"):
            conv.mix = blk.spectral.mix = mix
            out_c, out_b = conv(x), blk(x)
            assert out_c.shape == x.shape and out_c.dtype == BF and out_b.shape == x.shape and out_b.dtype == BF
            e_c, e_b = field_err(out_c, ref_c, 2), field_err(out_b, ref_b, 2)
            print(f"MEASURED sfno bf16 cpu {shape} mix={mix} conv {e_c:.3e} block {e_b:.3e}")
            assert e_c < TOL_LAYER and e_b < TOL_LAYER
    # the tables are cached per dtype beside the fp32 ones and follow the weights
    t16 = conv._degree_weight(BF)
    assert conv._degree_weight(BF) is t16 and t16.shape[0] == 1 and conv._degree_weight().shape[0] == 2
    assert MIX_CALLS and all(dt == (BF, BF, BF) for dt in MIX_CALLS)
    with torch.no_grad():
        conv.weight.mul_(2.0)
    assert conv._degree_weight(BF) is not t16
