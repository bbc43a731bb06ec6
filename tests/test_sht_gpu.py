"""Spherical harmonic transforms on the GPU: the ``legendre`` kernel (csrc/spectral/legendre.hip) against an fp64
einsum on the same fp32 inputs, ``sht`` / ``isht`` and the SFNO layers against the ``"torch"`` backend evaluated in
fp64, hipGraph capture and run-to-run determinism.  Everything runs under ``strict_mode`` with no fallback counted.

Error: relative L2 per field n (the maximum over fields, so one wrong column tile cannot be averaged away).
Bound: 1e-5, the project's bound for its bf16x3 kernels (tests/test_afno_mlp.py, tests/test_fno_channels.py)."""
import re

import pytest
import torch

from tensorrt_dft_plugins_amd import isht, sht, utils
from tensorrt_dft_plugins_amd.models.sfno import InverseRealSHT, RealSHT, SFNOBlock, SphericalConv2d
from tensorrt_dft_plugins_amd.ops import spectral as SP
from tensorrt_dft_plugins_amd.ops.sht import legendre_split

TOL = 1e-5

# (N, Q, R, M): everything ragged, one slab pair | several column tiles, slabs and row tiles | exactly aligned |
# more than 64 modes, R above Q | ragged last mode group.  All of these run on the 4-mode x 8-field tile (few
# workgroups); the next two fill the grid and reach the 4-mode x 16-field and the 8-mode x 16-field tiles; the last
# one (7 fields = 14 columns, 32 mode groups x 8 row groups = 256 workgroups, ragged in every dimension) reaches the
# 8-mode x 8-field tile.
CASES = [(3, 45, 23, 13), (40, 90, 90, 46), (2, 32, 16, 8), (1, 17, 70, 70), (5, 64, 64, 9),
         (128, 40, 100, 80), (128, 40, 200, 80), (7, 33, 500, 252)]
TILES = {(3, 45, 23, 13): (4, 1), (128, 40, 100, 80): (4, 2), (128, 40, 200, 80): (8, 2), (7, 33, 500, 252): (8, 1)}


def _field_err(out, ref, lead):
    """max over the ``lead`` leading (field) dims of the field's rel-L2 against the fp64 reference."""
    o = out.detach().cpu()
    if o.is_complex():
        o, ref = torch.view_as_real(o.to(torch.complex128)), torch.view_as_real(ref)
    o = o.double()
    n = 1
    for d in o.shape[:lead]:
        n *= d
    o, r = o.reshape(n, -1), ref.reshape(n, -1)
    num, den = (o - r).norm(dim=1), r.norm(dim=1)
    return float(torch.where(den > 0, num / den, num).max())


def _zeroed(table, tri):
    """The table with the part that ``tri`` declares zero set to zero."""
    M, R, Q = table.shape
    m = torch.arange(M)[:, None]
    t = table.clone()
    if tri == 1:
        t *= (torch.arange(R)[None, :] >= m)[:, :, None]
    elif tri == 2:
        t *= (torch.arange(Q)[None, :] >= m)[:, None, :]
    return t


_REF = {}


def _case(case):
    """(x, dense random table, {tri: fp64 product with the tri-zeroed table}) of one case, built once."""
    if case not in _REF:
        N, Q, R, M = case
        g = torch.Generator().manual_seed(N * 1000 + Q + R + M)
        x = torch.randn(N, Q, M, 2, generator=g)
        table = torch.randn(M, R, Q, generator=g) / Q ** 0.5
        refs = {tri: torch.einsum("mrq,nqmc->nrmc", _zeroed(table, tri).double(), x.double()) for tri in (0, 1, 2)}
        _REF[case] = (x, table, refs)
    return _REF[case]


@pytest.fixture()
def strict():
    prev = utils.strict_mode(True)
    SP.fallback_reset()
    try:
        yield
        assert SP.fallback_counts() == {}
    finally:
        utils.strict_mode(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_legendre_vs_fp64(device, strict, case, tri):
    """Tables that are truly zero where ``tri`` says so (the split table handed in, as the transforms do)."""
    N, Q, R, M = case
    x, table, refs = _case(case)
    if case in TILES:
        f = dict(re.findall(r"(\w+)=(\d+)", torch.ops.amd_dft.legendre_info(Q, R, M, 2 * N, tri)))
        assert (int(f["MT"]), int(f["CT"])) == TILES[case]
    t = _zeroed(table, tri).to(device)
    out = torch.ops.amd_dft.legendre(x.to(device), t, legendre_split(t), tri)
    assert out.shape == (N, R, M, 2) and out.dtype == torch.float32
    err = _field_err(out, refs[tri], 1)
    print(f"MEASURED legendre {case} tri={tri} {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_legendre_nonzero_in_skipped_part(device, strict, case, tri):
    """Random non-zero values where ``tri`` would allow skipping (the op splits the table itself here): ``tri = 0``
    must use them; ``tri = 1`` / ``2`` must give the product with that part zero, and under ``tri = 1`` the rows
    below m are exactly 0.0."""
    N, Q, R, M = case
    x, table, refs = _case(case)
    out = torch.ops.amd_dft.legendre(x.to(device), table.to(device), None, tri)
    err = _field_err(out, refs[tri], 1)
    print(f"MEASURED legendre dirty {case} tri={tri} {err:.3e}")
    assert err < TOL
    if tri == 0 and M > 1:
        # the dense product differs from both zeroed ones by far more than the bound: nothing was skipped
        assert _field_err(out, refs[1], 1) > 1e-2 and _field_err(out, refs[2], 1) > 1e-2
    if tri == 1:
        below = (torch.arange(R)[:, None] < torch.arange(M)[None, :])[None, :, :, None].expand(N, R, M, 2)
        assert torch.all(out.cpu()[below] == 0.0)


@pytest.mark.gpu
def test_legendre_view_and_leading_dims(device, strict):
    """[B, C, Q, M, 2] input taken as a view at an odd float offset (the op copies it to an 8-byte boundary)."""
    N, Q, R, M = CASES[0]
    x, table, refs = _case(CASES[0])
    buf = torch.zeros(x.numel() + 1, device=device)
    xv = buf[1:].view(1, N, Q, M, 2)
    xv.copy_(x)
    out = torch.ops.amd_dft.legendre(xv, table.to(device), None, 0)
    assert out.shape == (1, N, R, M, 2)
    assert _field_err(out[0], refs[0], 1) < TOL


@pytest.mark.gpu
def test_legendre_deterministic(device):
    x, table, _ = _case(CASES[1])
    xd, td = x.to(device), table.to(device)
    ts = legendre_split(td)
    a = torch.ops.amd_dft.legendre(xd, td, ts, 1)
    b = torch.ops.amd_dft.legendre(xd, td, ts, 1)
    assert torch.equal(a, b)


# (shape, lmax, mmax, grid)
SHT_CASES = [((2, 3, 45, 90), None, None, "legendre-gauss"), ((1, 20, 91, 180), 32, 32, "equiangular"),
             ((1, 2, 128, 256), None, 100, "equiangular")]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,lmax,mmax,grid", SHT_CASES, ids=["gauss45x90", "equi91x180_l32", "equi128x256_m100"])
def test_sht_isht_vs_fp64(device, strict, shape, lmax, mmax, grid):
    nlat, nlon = shape[-2:]
    g = torch.Generator().manual_seed(nlat)
    x = torch.randn(*shape, generator=g)
    fwd = RealSHT(nlat, nlon, lmax, mmax, grid, backend="torch")
    inv = InverseRealSHT(nlat, nlon, fwd.lmax, fwd.mmax, grid, backend="torch")
    ref = fwd(x.double())
    out = sht(x.to(device), lmax, mmax, grid)
    assert out.shape == (*shape[:2], fwd.lmax, fwd.mmax, 2)
    e_f = _field_err(torch.view_as_complex(out), ref, 2)
    # coefficients of a real field: random, zero where l < m, real at m = 0
    c = torch.randn(*shape[:2], fwd.lmax, fwd.mmax, 2, generator=g)
    c = c * (torch.arange(fwd.lmax)[:, None] >= torch.arange(fwd.mmax)[None, :])[:, :, None]
    c[..., 0, 1] = 0.0
    ref_i = inv(torch.view_as_complex(c.double()))
    out_i = isht(c.to(device), nlat, nlon, grid)
    assert out_i.shape == shape and out_i.dtype == torch.float32
    e_i = _field_err(out_i, ref_i, 2)
    print(f"MEASURED sht {shape} {grid} fwd {e_f:.3e} inv {e_i:.3e}")
    assert e_f < TOL
    assert e_i < TOL


def _layer_input():
    g = torch.Generator().manual_seed(46)
    return torch.randn(1, 20, 46, 90, generator=g)


@pytest.mark.gpu
def test_spherical_conv_and_block_vs_fp64(device, strict):
    torch.manual_seed(20)
    x = _layer_input()
    conv = SphericalConv2d(20, 20, 46, 90, backend="torch")
    blk = SFNOBlock(20, 46, 90, backend="torch")
    with torch.no_grad():
        ref_c = conv.double()(x.double())
        ref_b = blk.double()(x.double())
        conv, blk = conv.float().to(device).set_backend("amd"), blk.float().to(device).set_backend("amd")
        out_c, out_b = conv(x.to(device)), blk(x.to(device))
    assert out_c.shape == x.shape and out_b.shape == x.shape
    e_c, e_b = _field_err(out_c, ref_c, 2), _field_err(out_b, ref_b, 2)
    print(f"MEASURED sfno conv {e_c:.3e} block {e_b:.3e}")
    assert e_c < TOL
    assert e_b < TOL


@pytest.mark.gpu
def test_block_graph_capture(device, strict):
    torch.manual_seed(21)
    x = _layer_input().to(device)
    blk = SFNOBlock(20, 46, 90, backend="amd").to(device).eval()
    with torch.no_grad():
        eager = blk(x).clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = blk(x)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(y, eager)
