"""Vector spherical harmonic transforms on the GPU: the ``legendre_vec`` kernel (csrc/spectral/legendre.hip, VEC) in
both precisions and every shipped instance, ``vsht`` / ``ivsht`` and ``RealVectorSHT`` / ``InverseRealVectorSHT``
against the fp64 ``"torch"`` backend, and the contracts the spectral MFMA kernels are pinned to (guard bands, stale
LDS, the part ``tri`` declares zero, odd offsets, determinism, hipGraph replay).  References, cases and error models
are those of tests/test_vsht.py, built once there.  Everything runs under ``strict_mode`` with no fallback counted.

Kernel cases (N, Q, R, M): the three grids of ``GRIDS`` in the forward direction (all on the 4-mode x 4-field tile),
and one more per instance they do not reach -- each ragged in Q % 32, R % 16, M % MT and fields % (4 CT):
(9, 33, 200, 127) fills 256 workgroups of the 4 x 8 tile in both precisions; (9, 33, 200, 252) the bf16 8 x 8 tile;
(3, 33, 500, 252), 12 columns, the bf16 8 x 4 tile.

Bounds: fp32 1e-5 per (field, component) (tests/test_sht_gpu.py); bf16 kernel: every element within
2^-8 |ref| + 2 ceil32(Q) 2^-22 (sum |a||x0| + sum |b||x1|) of the exact product of the same bf16 operands; bf16
transforms 2e-2 per field."""
import pytest
import torch

import test_kernel_bounds_gpu as KB
import test_vsht as V
from tensorrt_dft_plugins_amd import ivsht, utils, vsht
from tensorrt_dft_plugins_amd.models.sfno import InverseRealVectorSHT, RealVectorSHT
from tensorrt_dft_plugins_amd.ops import spectral as SP
from tensorrt_dft_plugins_amd.ops.sht import legendre_split

BF = torch.bfloat16
ops = torch.ops.amd_dft
DT = {"fp32": torch.float32, "bf16": BF}
# (nlat, nlon, lmax, mmax, fields, grid)
GRIDS = [(33, 64, 20, 9, 3, "legendre-gauss"), (25, 48, 13, 13, 17, "equiangular"), (70, 40, 70, 21, 2, "legendre-gauss")]
BASE = [(f, nlat, lmax, mmax) for nlat, _, lmax, mmax, f, _ in GRIDS]
assert BASE == V.OP_CASES
# case -> {bf16?: (MT, CT)}: the instance each precision must take (absent: that precision does not run the case)
CASES = {BASE[0]: {False: (4, 1), True: (4, 1)}, BASE[1]: {False: (4, 1), True: (4, 1)},
         BASE[2]: {False: (4, 1), True: (4, 1)}, (9, 33, 200, 127): {False: (4, 2), True: (4, 2)},
         (9, 33, 200, 252): {True: (8, 2)}, (3, 33, 500, 252): {True: (8, 1)}}
SHIPPED = {(False, 4, 2), (False, 4, 1), (True, 8, 2), (True, 8, 1), (True, 4, 2), (True, 4, 1)}
RUNS = [(c, p) for c, inst in CASES.items() for p in ("fp32", "bf16") if (p == "bf16") in inst]
rid = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


@pytest.fixture()
def strict():
    prev = utils.strict_mode(True)
    SP.fallback_reset()
    try:
        yield
        assert SP.fallback_counts() == {}
    finally:
        utils.strict_mode(prev)


def _route(case, prec, tri):
    N, Q, R, M = case
    bf = prec == "bf16"
    f = V.fields(ops.legendre_vec_info(Q, R, M, 4 * N, tri, bf))
    assert (f["MT"], f["CT"]) == CASES[case][bf], f
    assert Q % 32 and R % 16 and M % f["MT"] and N % (4 * f["CT"])
    return f


def test_every_shipped_instance_is_reached():
    """The instances the launcher can dispatch to (legendre_route with vec: fp32 4 x {2, 1}, bf16 {8, 4} x {2, 1}) are all
    among the cases above, by the info string the launcher's own route function answers."""
    seen = set()
    for case, prec in RUNS:
        f = _route(case, prec, 0)
        seen.add((prec == "bf16", f["MT"], f["CT"]))
    assert seen == SHIPPED


def _check(out, case, prec, tri, what):
    N, Q, R, M = case
    _, _, _, refs, sums = V.op_case(case, prec == "bf16")
    assert out.shape == (N, 2, R, M, 2) and out.dtype == DT[prec]
    if prec == "bf16":
        V.assert_bf16_product(out, refs[tri], sums[tri], Q, f"legendre_vec bf16 {what} {case} tri={tri}")
    else:
        err = V.field_err(out, refs[tri], 2)
        print(f"MEASURED legendre_vec fp32 {what} {case} tri={tri} {err:.3e}")
        assert err < V.TOL
    if tri == 1:
        assert torch.all(out.cpu()[V.below_rows(N, R, M)] == 0.0)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case,prec", RUNS, ids=rid)
def test_legendre_vec_vs_fp64(device, strict, case, prec, tri):
    """Dense random tables, non-zero where ``tri`` would allow skipping, split by the op itself: ``tri = 0`` must use
    that part (the result is far from both zeroed products), ``tri = 1`` / ``2`` give the product with it zero."""
    _route(case, prec, tri)
    x, ta, tb, refs, _ = V.op_case(case, prec == "bf16")
    out = ops.legendre_vec(x.to(device), ta.to(device), tb.to(device), None, None, tri)
    _check(out, case, prec, tri, "dirty")
    if tri == 0:
        assert V.field_err(out, refs[1], 2) > 1e-2 and V.field_err(out, refs[2], 2) > 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", BASE, ids=rid)
def test_legendre_vec_with_zero_b_is_legendre(device, strict, case, prec, tri):
    """The two ops are instances of one kernel: with B = 0 the vector instance adds exact zeros between the scalar
    instance's MFMAs, in the same accumulation order whatever tile either route picks, so the result is bit for bit
    ``legendre`` of the same table over the 2 N component planes."""
    N, Q, R, M = case
    x, ta, _, _, _ = V.op_case(case, prec == "bf16")
    xd, tad = x.to(device), ta.to(device)
    out = ops.legendre_vec(xd, tad, torch.zeros_like(tad), None, None, tri)
    ref = ops.legendre(xd.view(2 * N, Q, M, 2), tad, None, tri)
    assert torch.equal(out, ref.view(N, 2, R, M, 2))


def _guarded(device, case, prec, tri, x=None):
    N, Q, R, M = case
    x0, ta, tb, _, _ = V.op_case(case, prec == "bf16")
    ta, tb = V.zeroed(ta, tri), V.zeroed(tb, tri)
    gx = KB.Guarded(device, 0, x0 if x is None else x)
    ga, gb = KB.Guarded(device, 1, ta), KB.Guarded(device, 2, tb)
    gas = KB.Guarded(device, 3, legendre_split(ta.to(device)).cpu())
    gbs = KB.Guarded(device, 4, legendre_split(tb.to(device)).cpu())
    gy = KB.Guarded(device, 5, shape=(N, 2, R, M, 2), dtype=DT[prec])
    return [gx, ga, gb, gas, gbs], gy


@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case,prec", RUNS, ids=rid)
def test_legendre_vec_guard_bands(device, strict, case, prec, tri):
    """Every tensor a view between 4096-element NaN-pattern bands, the output included (legendre_vec_out); bands and
    inputs are compared bit for bit afterwards."""
    _route(case, prec, tri)
    inputs, gy = _guarded(device, case, prec, tri)
    assert ops.legendre_vec_out(*(g.view for g in inputs), tri, gy.view) is gy.view
    KB._check_untouched(inputs, gy)
    _check(gy.view, case, prec, tri, "guarded")


@pytest.mark.gpu
@KB.lds
@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case,prec", RUNS, ids=rid)
def test_legendre_vec_stale_lds(device, case, prec, tri):
    """q >= Q, planes >= 2 N and m >= M of the slab image must be written as zeros (every case is ragged in all
    three): the kernel launched right after ``lds_poison()`` still gives the clean result."""
    _route(case, prec, tri)
    inputs, gy = _guarded(device, case, prec, tri)
    args = [g.view for g in inputs]
    KB._poison_then(lambda: ops.legendre_vec_out(*args, tri, gy.view))
    ops.legendre_vec_out(*args, tri, gy.view)
    assert torch.isfinite(gy.view.float()).all()
    _check(gy.view, case, prec, tri, "stale-lds")


@pytest.mark.gpu
@KB.lds
def test_lds_poison_reaches_the_next_kernel(device):
    """The premise of the stale-LDS tests, checked here as tests/test_kernel_bounds_gpu.py does."""
    ops.lds_poison()
    assert float(ops.lds_probe()) == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("case,prec", [r for r in RUNS if r[0] in (BASE[1], BASE[2])], ids=rid)
def test_legendre_vec_poison_where_tri2_declares_zero(device, strict, case, prec, poison):
    N, Q, R, M = case
    x, ta, tb, _, _ = V.op_case(case, prec == "bf16")
    xp = torch.where(V.below_cols(N, Q, M), poison, x.float()).to(DT[prec]).to(device)
    out = ops.legendre_vec(xp, ta.to(device), tb.to(device), None, None, 2)
    assert torch.isfinite(out.float()).all()
    _check(out, case, prec, 2, f"poison {poison}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_legendre_vec_odd_offset_view_and_misaligned_out(device, strict, prec):
    """An ``x`` view one element into its storage is copied to a pair boundary; an ``out`` there raises instead."""
    case = BASE[0]
    N, Q, R, M = case
    x, ta, tb, _, _ = V.op_case(case, prec == "bf16")
    buf = torch.zeros(x.numel() + 1, device=device, dtype=DT[prec])
    xv = buf[1:].view(1, N, 2, Q, M, 2)
    xv.copy_(x)
    assert xv.data_ptr() % (2 * xv.element_size()) != 0
    tad, tbd = ta.to(device), tb.to(device)
    out = ops.legendre_vec(xv, tad, tbd, None, None, 0)
    assert out.shape == (1, N, 2, R, M, 2)
    _check(out[0], case, prec, 0, "odd offset")
    ybuf = torch.empty(N * 2 * R * M * 2 + 1, device=device, dtype=DT[prec])
    for bad in (ybuf[1:].view(N, 2, R, M, 2), torch.empty(N, 2, R, M, 4, device=device, dtype=DT[prec])[..., ::2],
                torch.empty(N, 2, R, M, 2, dtype=DT[prec])):
        with pytest.raises(RuntimeError, match="out must"):
            ops.legendre_vec_out(x.to(device), tad, tbd, None, None, 0, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("case,prec", [(BASE[2], "fp32"), (BASE[2], "bf16"), ((9, 33, 200, 252), "bf16")], ids=rid)
def test_legendre_vec_deterministic_and_graph_replay(device, case, prec):
    x, ta, tb, _, _ = V.op_case(case, prec == "bf16")
    xd, tad, tbd = x.to(device), ta.to(device), tb.to(device)
    sa, sb = legendre_split(tad), legendre_split(tbd)
    a = ops.legendre_vec(xd, tad, tbd, sa, sb, 1)
    b = ops.legendre_vec(xd, tad, tbd, sa, sb, 1)
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = ops.legendre_vec(xd, tad, tbd, sa, sb, 1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, a)


# ------------------------------------------------------------------------------------------------ the transforms
@pytest.mark.gpu
@pytest.mark.parametrize("g", GRIDS, ids=rid)
def test_vsht_ivsht_vs_fp64(device, strict, g):
    """fp32 and bf16 ``vsht`` / ``ivsht`` and the two modules against the fp64 torch backend on the same inputs: a
    random field forward, random coefficients of a real field inverse, as tests/test_sht_gpu.py does.

    The forward input is not the band-limited field of the CPU tier.  The bf16x3 product keeps 16 significant bits of
    each operand, so its error is about 3.5e-6 of sum |W| |v|, and 1e-5 of the result only while the sum cancels little.
    Emulating the split in fp64 on the host (hi and lo planes rounded as the kernel rounds them, products exact) gives,
    for the forward table at (70, 40, 70, 21): 4.3e-6 per field on a random field, 1.15e-5 on a field synthesised from
    white coefficients up to l = 69 (sum |W| |v| is 17 times the result there); the kernel measured 1.08e-5 on that
    field.  At the other two grids the emulation gives 5.5e-6 to 6.3e-6 for either input."""
    nlat, nlon, lmax, mmax, nf, grid = g
    vg = (grid, nlat, nlon, lmax, mmax)
    _, c, _, ref_i = V.transform_case(vg, (1, nf))
    fwd, inv = V.pair(vg)
    v = torch.randn(1, nf, 2, nlat, nlon, generator=torch.Generator().manual_seed(nlat))
    ref_f = fwd(v.double())
    out = vsht(v.to(device), lmax, mmax, grid)
    out_i = ivsht(c.to(device), nlat, nlon, grid)
    assert out.shape == (1, nf, 2, lmax, mmax, 2) and out.dtype == torch.float32
    assert out_i.shape == (1, nf, 2, nlat, nlon) and out_i.dtype == torch.float32
    e_f, e_i = V.field_err(out, torch.view_as_real(ref_f), 2), V.field_err(out_i, ref_i, 2)
    print(f"MEASURED vsht fp32 {g} fwd {e_f:.3e} inv {e_i:.3e}")
    assert e_f < V.TOL
    assert e_i < V.TOL
    mf = RealVectorSHT(nlat, nlon, lmax, mmax, grid).to(device)
    mi = InverseRealVectorSHT(nlat, nlon, lmax, mmax, grid).to(device)
    cm = mf(v.to(device))
    assert cm.dtype == torch.complex64 and torch.equal(torch.view_as_real(cm), out)
    assert torch.equal(mi(torch.view_as_complex(c.to(device))), out_i)
    vb, cb = v.to(BF), c.to(BF)
    ob, oib = vsht(vb.to(device), lmax, mmax, grid), ivsht(cb.to(device), nlat, nlon, grid)
    assert ob.dtype == BF and oib.dtype == BF and ob.shape == out.shape and oib.shape == out_i.shape
    e_fb = V.field_err(ob, torch.view_as_real(fwd(vb.double())), 2)
    e_ib = V.field_err(oib, inv(torch.view_as_complex(cb.double())), 2)
    print(f"MEASURED vsht bf16 {g} fwd {e_fb:.3e} inv {e_ib:.3e}")
    assert e_fb < V.TOL_BF16
    assert e_ib < V.TOL_BF16
