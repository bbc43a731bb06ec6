"""The bf16 precision of the spherical line on the GPU: the bf16 instances of the ``legendre`` and ``sfno_mix`` kernels
(csrc/spectral/legendre.hip, sfno_mix.hip), ``sht`` / ``isht`` and the SFNO layers on bf16 tensors.  Everything runs
under ``strict_mode`` with no fallback counted.

Kernel tests, at the case lists of tests/test_sht_gpu.py, tests/test_sfno_mix_gpu.py and tests/test_kernel_bounds_gpu.py
(all four Legendre tilings, ragged slab / row / mode / column edges, every ``sfno_mix`` route) and every ``tri``:

1. elementwise against the exact product of the same bf16 operands, |out - ref| <= 2^-8 |ref| + K 2^-22 S
   (tests/test_sfno_bf16.py derives it);
2. per field against the fp64 product with the unrounded fp32 table / weights: 1e-2;
3. the contracts the fp32 kernels are pinned to: exact zeros, the declared-zero part ignored (table values, NaN / Inf
   in the input), guard bands around every tensor of an ``_out`` call, stale LDS, views at an odd element offset,
   run-to-run determinism and hipGraph replay.

Transform and layer tests: against the ``"torch"`` backend in fp64 on the same bf16 inputs and bf16-rounded weights,
max per-field rel-L2 < 2e-2 (the project's bf16 layer bound; a CPU emulation of the rounding chains gives about 3e-3 for
the transforms and the block and 5e-3 for the convolution).  Shapes: [2, 5, 33, 64] equiangular, untruncated, and
[1, 20, 45, 90] Legendre-Gauss with lmax 23, mmax 13.  Which routes the bf16 layers rely on, and how each is checked:
the longitude passes at nlon 64 and 90 are Stockham hand kernels with bf16 loads and stores (every length that fits
LDS is; ``fft_pass_info`` only rules out the composed ``large`` route, and ``strict_mode`` with no fallback counted is
what shows the calls stayed on them), so neither length had to be replaced; ``fno_mix`` is NOT native in bf16 (the op
upcasts its operands and mixes in fp32, which no fallback counter sees), so the bf16 layers mix with ``sfno_mix`` under
``mix="auto"`` too, and ``test_layers_bf16`` pins that: ``fno_mix`` or the expansion fail it, and every mix call must
be ``sfno_mix`` on bf16 tensors."""
import re

import pytest
import torch

import test_kernel_bounds_gpu as KB
import test_sfno_bf16 as T
import test_sfno_mix_gpu as MIX
import test_sht_gpu as LEG
from tensorrt_dft_plugins_amd import isht, sht, utils
from tensorrt_dft_plugins_amd.models import sfno
from tensorrt_dft_plugins_amd.ops import spectral as SP
from tensorrt_dft_plugins_amd.ops.sht import legendre_split

BF = torch.bfloat16
ops = torch.ops.amd_dft
ids = lambda c: "x".join(map(str, c))  # noqa: E731


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


def _check_legendre(out, case, tri, what):
    N, Q, R, M = case
    _, _, _, exact, unrounded = T.legendre_case(case)
    assert out.shape[-4:] == (N, R, M, 2) and out.dtype == BF
    o = out.reshape(N, R, M, 2)
    T.assert_exact_product(o, *exact[tri], T.ceil_to(Q, 32), f"legendre {what} {case} tri={tri}")
    err = T.field_err(o, unrounded[tri], 1)
    print(f"MEASURED legendre bf16 {what} {case} tri={tri} vs unrounded table {err:.3e}")
    assert err < T.TOL_KERNEL
    if tri == 1:
        below = (torch.arange(R)[:, None] < torch.arange(M)[None, :])[None, :, :, None].expand(N, R, M, 2)
        assert torch.all(o.cpu()[below] == 0.0)


def _check_mix(out, case, tri, what):
    B, Cin, Cout, L, M = case
    _, _, _, exact, unrounded = T.mix_case(case)
    assert out.shape == (B, Cout, L, M, 2) and out.dtype == BF
    T.assert_exact_product(out, *exact[tri], T.ceil_to(2 * Cin, 32), f"sfno_mix {what} {case} tri={tri}")
    err = T.field_err(out, unrounded[tri], 2)
    print(f"MEASURED sfno_mix bf16 {what} {case} tri={tri} vs unrounded weights {err:.3e}")
    assert err < T.TOL_KERNEL
    if tri == 1:
        assert torch.all(out.cpu()[(~T.keep(L, M))[None, None].expand(B, Cout, L, M, 2)] == 0.0)


# ------------------------------------------------------------------------------------------------ legendre
@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case", LEG.CASES, ids=ids)
def test_legendre_bf16(device, strict, case, tri):
    """Tables that are truly zero where ``tri`` says so, the one-plane split handed in (as the transforms do); the
    tiling is the fp32 one."""
    N, Q, R, M = case
    x, _, tb, _, _ = T.legendre_case(case)
    f = _fields(ops.legendre_info(Q, R, M, 2 * N, tri, True))
    assert f["bf16"] == 1
    if case in LEG.TILES:
        assert (f["MT"], f["CT"]) == LEG.TILES[case]
    t = T.zeroed(tb, tri).to(device)
    _check_legendre(ops.legendre(x.to(device), t, legendre_split(t), tri), case, tri, "clean")


@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case", LEG.CASES, ids=ids)
def test_legendre_bf16_nonzero_in_skipped_part(device, strict, case, tri):
    """Random non-zero values where ``tri`` would allow skipping (the op pads the table itself here): ``tri = 0`` uses
    them; ``tri = 1`` / ``2`` give the product with that part zero, rows below m exactly 0.0 under ``tri = 1``."""
    N, Q, R, M = case
    x, _, tb, _, unrounded = T.legendre_case(case)
    out = ops.legendre(x.to(device), tb.to(device), None, tri)
    _check_legendre(out, case, tri, "dirty")
    if tri == 0 and M > 1:
        assert T.field_err(out, unrounded[1], 1) > 1e-1 and T.field_err(out, unrounded[2], 1) > 1e-1


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("case", LEG.CASES[:2], ids=ids)
def test_legendre_bf16_poison_where_tri2_declares_zero(device, strict, case, poison):
    N, Q, R, M = case
    x, _, tb, _, _ = T.legendre_case(case)
    below = (torch.arange(Q)[:, None] < torch.arange(M)[None, :])[None, :, :, None].expand(N, Q, M, 2)
    xp = torch.where(below, poison, x.float()).to(BF).to(device)
    t = T.zeroed(tb, 2).to(device)
    _check_legendre(ops.legendre(xp, t, legendre_split(t), 2), case, 2, f"poison {poison}")


def _leg_guarded(device, case, tri):
    N, Q, R, M = case
    f = _fields(ops.legendre_info(Q, R, M, 2 * N, tri, True))
    assert (f["MT"], f["CT"]) == KB.LEG_CASES[case] and Q % 32 and R % 16 and M % f["MT"] and N % (8 * f["CT"])
    x, _, tb, _, _ = T.legendre_case(case)
    t = T.zeroed(tb, tri)
    gx, gt, gs = KB.Guarded(device, 0, x), KB.Guarded(device, 1, t), KB.Guarded(device, 2, legendre_split(t))
    gy = KB.Guarded(device, 3, shape=(N, R, M, 2), dtype=BF)
    return gx, gt, gs, gy


@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case", list(KB.LEG_CASES), ids=ids)
def test_legendre_bf16_guard_bands(device, strict, case, tri):
    """``legendre_out`` on views inside NaN-patterned buffers (x, the table, the one plane, y), one shape per tiling,
    ragged in every tiled dimension: every guard and input bitwise unchanged, the result finite and right."""
    gx, gt, gs, gy = _leg_guarded(device, case, tri)
    assert ops.legendre_out(gx.view, gt.view, gs.view, tri, gy.view) is gy.view
    KB._check_untouched([gx, gt, gs], gy)
    _check_legendre(gy.view, case, tri, "guarded")


@pytest.mark.gpu
@KB.lds
@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case", list(KB.LEG_CASES), ids=ids)
def test_legendre_bf16_stale_lds(device, strict, case, tri):
    """q >= Q, n >= N and m >= M of the one-plane slab image must be written as zeros: the launch right after an
    ``lds_poison()`` fill gives the same finite result."""
    gx, gt, gs, gy = _leg_guarded(device, case, tri)
    KB._poison_then(lambda: ops.legendre_out(gx.view, gt.view, gs.view, tri, gy.view))
    ops.legendre_out(gx.view, gt.view, gs.view, tri, gy.view)
    assert torch.isfinite(gy.view.float()).all()
    _check_legendre(gy.view, case, tri, "stale-lds")


@pytest.mark.gpu
def test_legendre_bf16_view_at_odd_offset_and_out_alignment(device, strict):
    """[B, C, Q, M, 2] input as a view at an odd bf16 element offset (the op copies it to a 4-byte boundary); an
    ``out`` there is refused, one on a 4-byte boundary that is not an 8-byte one is taken."""
    case = LEG.CASES[0]
    N, Q, R, M = case
    x, _, tb, _, _ = T.legendre_case(case)
    buf = torch.zeros(x.numel() + 1, device=device, dtype=BF)
    xv = buf[1:].view(1, N, Q, M, 2)
    xv.copy_(x)
    assert xv.data_ptr() % 4 == 2
    td = tb.to(device)
    for tri in (0, 2):
        out = ops.legendre(xv, td, None, tri)
        assert out.shape == (1, N, R, M, 2)
        _check_legendre(out, case, tri, "odd view")
    ybuf = torch.zeros(N * R * M * 2 + 2, device=device, dtype=BF)
    with pytest.raises(RuntimeError, match="4-byte"):
        ops.legendre_out(x.to(device), td, None, 0, ybuf[1:-1].view(N, R, M, 2))
    y2 = ybuf[2:].view(N, R, M, 2)
    assert y2.data_ptr() % 8 == 4
    _check_legendre(ops.legendre_out(x.to(device), td, None, 0, y2), case, 0, "out at 4 mod 8")


@pytest.mark.gpu
def test_legendre_bf16_deterministic_and_graph(device, strict):
    """Two runs are bit-identical, and one hipGraph capture replays to the eager result."""
    x, _, tb, _, _ = T.legendre_case(LEG.CASES[1])
    xd, td = x.to(device), tb.to(device)
    ts = legendre_split(td)
    for tri in (1, 2):
        a = ops.legendre(xd, td, ts, tri)
        assert torch.equal(a, ops.legendre(xd, td, ts, tri))
    eager = ops.legendre(xd, td, ts, 1).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = ops.legendre(xd, td, ts, 1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)


# ------------------------------------------------------------------------------------------------ sfno_mix
@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("case", MIX.CASES, ids=ids)
def test_sfno_mix_bf16(device, strict, case, tri):
    """Spectra that are truly zero where ``tri`` says so, the one-plane table handed in (as the layers do)."""
    B, Cin, Cout, L, M = case
    c, _, wb, _, _ = T.mix_case(case)
    f = _fields(ops.sfno_mix_info(B, Cin, Cout, L, M, 0, True))
    assert (f["slabs"], f["otiles"], f["ogroups"], f["ctiles"]) == MIX.SHAPE[case] and f["coltile"] == 64
    assert f["bf16"] == 1 and f["lds"] == 128 * 80
    cz = (c * T.keep(L, M) if tri else c).to(device)
    wd = wb.to(device)
    _check_mix(SP.sfno_mix(cz, wd, SP.sfno_mix_split(wd), tri), case, tri, "clean")


@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("case", MIX.CASES, ids=ids)
def test_sfno_mix_bf16_nonzero_where_l_below_m(device, strict, case, tri):
    """Random non-zero input where l < m (the op repacks the weights itself here): ``tri = 0`` uses it; ``tri = 1``
    gives the product of the zeroed spectrum, exact 0.0 there."""
    c, _, wb, _, unrounded = T.mix_case(case)
    out = SP.sfno_mix(c.to(device), wb.to(device), None, tri)
    _check_mix(out, case, tri, "dirty")
    if tri == 0 and case[4] > 1:
        assert T.field_err(out, unrounded[1], 2) > 1e-1


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("case", MIX.CASES[:2], ids=ids)
def test_sfno_mix_bf16_poison_where_l_below_m(device, strict, case, poison):
    B, Cin, Cout, L, M = case
    c, _, wb, _, _ = T.mix_case(case)
    k = T.keep(L, M)[None, None].expand(B, Cin, L, M, 2)
    cp = torch.where(k, c.float(), poison).to(BF).to(device)
    wd = wb.to(device)
    _check_mix(SP.sfno_mix(cp, wd, SP.sfno_mix_split(wd), 1), case, 1, f"poison {poison}")


def _mix_guarded(device, case, tri):
    B, Cin, Cout, L, M = case
    c, _, wb, _, _ = T.mix_case(case)
    gc = KB.Guarded(device, 0, c * T.keep(L, M) if tri else c)
    gw, gs = KB.Guarded(device, 1, wb), KB.Guarded(device, 2, SP.sfno_mix_split(wb))
    gy = KB.Guarded(device, 3, shape=(B, Cout, L, M, 2), dtype=BF)
    return gc, gw, gs, gy


@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("case", KB.MIX_CASES, ids=ids)
def test_sfno_mix_bf16_guard_bands(device, strict, case, tri):
    gc, gw, gs, gy = _mix_guarded(device, case, tri)
    assert ops.sfno_mix_out(gc.view, gw.view, gs.view, tri, gy.view) is gy.view
    KB._check_untouched([gc, gw, gs], gy)
    _check_mix(gy.view, case, tri, "guarded")


@pytest.mark.gpu
@KB.lds
@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("case", [MIX.CASES[1], MIX.CASES[4]], ids=ids)
def test_sfno_mix_bf16_stale_lds(device, strict, case, tri):
    """i >= Cin and dead columns of the one-plane slab image must be written as zeros."""
    gc, gw, gs, gy = _mix_guarded(device, case, tri)
    KB._poison_then(lambda: ops.sfno_mix_out(gc.view, gw.view, gs.view, tri, gy.view))
    ops.sfno_mix_out(gc.view, gw.view, gs.view, tri, gy.view)
    assert torch.isfinite(gy.view.float()).all()
    _check_mix(gy.view, case, tri, "stale-lds")


@pytest.mark.gpu
def test_sfno_mix_bf16_view_at_odd_offset_and_out_alignment(device, strict):
    case = MIX.CASES[1]
    B, Cin, Cout, L, M = case
    c, _, wb, _, _ = T.mix_case(case)
    buf = torch.zeros(c.numel() + 1, device=device, dtype=BF)
    cv = buf[1:].view(c.shape)
    cv.copy_(c)
    assert cv.data_ptr() % 4 == 2
    wd = wb.to(device)
    ws = SP.sfno_mix_split(wd)
    for tri in (0, 1):
        _check_mix(SP.sfno_mix(cv, wd, ws, tri), case, tri, "odd view")
    ybuf = torch.zeros(B * Cout * L * M * 2 + 2, device=device, dtype=BF)
    with pytest.raises(RuntimeError, match="4-byte"):
        ops.sfno_mix_out(c.to(device), wd, ws, 0, ybuf[1:-1].view(B, Cout, L, M, 2))
    y2 = ybuf[2:].view(B, Cout, L, M, 2)
    assert y2.data_ptr() % 8 == 4
    _check_mix(ops.sfno_mix_out(c.to(device), wd, ws, 0, y2), case, 0, "out at 4 mod 8")


@pytest.mark.gpu
def test_sfno_mix_bf16_split_on_device_deterministic_and_graph(device, strict):
    c, _, wb, _, _ = T.mix_case(MIX.CASES[4])
    cd, wd = c.to(device), wb.to(device)
    ws = SP.sfno_mix_split(wd)
    assert torch.equal(ws.cpu(), SP.sfno_mix_split(wb))
    for tri in (0, 1):
        assert torch.equal(SP.sfno_mix(cd, wd, ws, tri), SP.sfno_mix(cd, wd, ws, tri))
    eager = SP.sfno_mix(cd, wd, ws, 1).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = SP.sfno_mix(cd, wd, ws, 1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)


# ------------------------------------------------------------------------------------------------ transforms, layers
def _native_passes(shape, mmax):
    """The bf16 longitude passes of this shape are single LDS-resident Stockham passes, not the composed ``large``
    route (host query; it describes the unpruned pass and cannot see a fallback: the ``strict`` fixture does that)."""
    nlat, nlon = shape[-2:]
    r2c = ops.fft_pass_info("r2c", list(shape), len(shape) - 1, nlon, True, True)
    c2r = ops.fft_pass_info("c2r", [*shape[:-1], mmax], len(shape) - 1, nlon, True, True)
    assert r2c.split()[0] in ("fixed", "generic") and c2r.split()[0] in ("fixed", "generic"), (r2c, c2r)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,lmax,mmax,grid", T.SHT_CASES, ids=T.SHT_IDS)
def test_sht_isht_bf16(device, strict, shape, lmax, mmax, grid):
    nlat, nlon = shape[-2:]
    x, ref, c, ref_i, (L, M) = T.sht_refs(shape, lmax, mmax, grid)
    _native_passes(shape, M)
    out = sht(x.to(device), lmax, mmax, grid)
    assert out.shape == (*shape[:2], L, M, 2) and out.dtype == BF
    assert torch.all(out.cpu()[(~T.keep(L, M)).expand(*shape[:2], L, M, 2)] == 0.0)
    out_i = isht(c.to(device), nlat, nlon, grid)
    assert out_i.shape == shape and out_i.dtype == BF
    e_f, e_i = T.field_err(out, ref, 2), T.field_err(out_i, ref_i, 2)
    print(f"MEASURED sht bf16 {shape} {grid} fwd {e_f:.3e} inv {e_i:.3e}")
    assert e_f < T.TOL_LAYER
    assert e_i < T.TOL_LAYER


@pytest.mark.gpu
@pytest.mark.parametrize("shape,lmax,mmax,grid", T.SHT_CASES, ids=T.SHT_IDS)
def test_layers_bf16(device, strict, shape, lmax, mmax, grid, monkeypatch):
    """``SphericalConv2d`` under both ``mix`` values and ``SFNOBlock`` on a bf16 input: bf16 out, within the layer
    bound of the fp64 torch backend, the two mixes within the bound of each other.  Under both values the mix is
    ``sfno_mix`` on bf16 tensors with the one-plane table; ``fno_mix`` (no bf16 kernel) or the expansion fail the
    test, although the expansion is far below the limit at these shapes."""
    x, conv, blk, ref_c, ref_b = T.layer_refs(shape, lmax, mmax, grid)
    _native_passes(shape, conv.sht.mmax)
    assert conv.expanded_bytes() < sfno.EXPAND_LIMIT_BYTES
    T.pin_bf16_mix(monkeypatch, [conv, blk.spectral])
    conv, blk, xd = conv.to(device), blk.to(device), x.to(device)
    outs = {}
    with torch.no_grad():
        for mix in ("auto", "degree"):
            conv.mix = blk.spectral.mix = mix
            out_c, out_b = conv(xd), blk(xd)
            assert out_c.shape == x.shape and out_c.dtype == BF and out_b.shape == x.shape and out_b.dtype == BF
            e_c, e_b = T.field_err(out_c, ref_c, 2), T.field_err(out_b, ref_b, 2)
            print(f"MEASURED sfno bf16 {shape} mix={mix} conv {e_c:.3e} block {e_b:.3e}")
            assert e_c < T.TOL_LAYER
            assert e_b < T.TOL_LAYER
            outs[mix] = (out_c, out_b)
    assert len(T.MIX_CALLS) == 4 and all(dt == (BF, BF, BF) for dt in T.MIX_CALLS)
    for a, d in zip(outs["auto"], outs["degree"]):
        assert T.field_err(d, a.cpu().double(), 2) < T.TOL_LAYER


@pytest.mark.gpu
@pytest.mark.parametrize("mix", ["auto", "degree"])
def test_block_bf16_graph_capture(device, strict, mix):
    shape, lmax, mmax, grid = T.SHT_CASES[1]
    x, _, blk, _, _ = T.layer_refs(shape, lmax, mmax, grid, seed=21)
    blk.spectral.mix = mix
    blk, xd = blk.to(device).eval(), x.to(device)
    with torch.no_grad():
        eager = blk(xd).clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = blk(xd)
        g.replay()
        torch.cuda.synchronize()
    assert y.dtype == BF and torch.equal(y, eager)
