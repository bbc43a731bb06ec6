"""SFNO per-degree channel mixing on the GPU: the ``sfno_mix`` kernel (csrc/spectral/sfno_mix.hip) against an fp64
complex einsum on the same fp32 inputs, the SFNO layers on it against the ``"torch"`` backend evaluated in fp64,
hipGraph capture and run-to-run determinism.  Everything runs under ``strict_mode`` with no fallback counted.

Error: relative L2 per (b, o) field (the maximum over fields, so one wrong tile cannot be averaged away).
Bound: 1e-5, the project's bound for one bf16x3 kernel (tests/test_sht_gpu.py, tests/test_afno_mlp.py)."""
import re

import pytest
import torch

from tensorrt_dft_plugins_amd import utils
from tensorrt_dft_plugins_amd.models import sfno
from tensorrt_dft_plugins_amd.models.sfno import SFNOBlock, SphericalConv2d
from tensorrt_dft_plugins_amd.ops import spectral as SP

TOL = 1e-5

# (B, Cin, Cout, L, M): one ragged slab, Cout < 16 | two slabs, ragged second row tile | exactly aligned, a full
# 64-row group | M > L, ragged second row group, odd M | several column tiles per degree, batch-packed columns at
# low l | nine slabs, the last one ragged.  The route has one tiling (64 complex columns), asserted per case.
CASES = [(1, 3, 5, 7, 5), (2, 20, 20, 23, 13), (3, 32, 64, 16, 16), (1, 40, 72, 9, 33), (5, 16, 16, 70, 70),
         (2, 130, 24, 12, 12)]
# what each case must reach: (slabs, otiles, ogroups, column tiles of the fullest degree at tri = 0)
SHAPE = {(1, 3, 5, 7, 5): (1, 1, 1, 1), (2, 20, 20, 23, 13): (2, 2, 1, 1), (3, 32, 64, 16, 16): (2, 4, 1, 1),
         (1, 40, 72, 9, 33): (3, 5, 2, 1), (5, 16, 16, 70, 70): (1, 1, 1, 6), (2, 130, 24, 12, 12): (9, 2, 1, 1)}


def _field_err(out, ref):
    """max over the (b, o) fields of the field's rel-L2 against the fp64 reference."""
    o = out.detach().cpu().double()
    n = o.shape[0] * o.shape[1]
    o, r = o.reshape(n, -1), ref.reshape(n, -1)
    num, den = (o - r).norm(dim=1), r.norm(dim=1)
    return float(torch.where(den > 0, num / den, num).max())


def _keep(L, M):
    return (torch.arange(L)[:, None] >= torch.arange(M)[None, :])[:, :, None]


_REF = {}


def _case(case):
    """(c random everywhere, w, {tri: fp64 product, with c zeroed where l < m for tri = 1}) of one case, built once."""
    if case not in _REF:
        B, Cin, Cout, L, M = case
        g = torch.Generator().manual_seed(sum(case))
        c = torch.randn(B, Cin, L, M, 2, generator=g)
        w = torch.randn(Cin, Cout, L, 2, generator=g) / Cin ** 0.5
        y = torch.view_as_real(torch.einsum("bilm,iol->bolm", torch.view_as_complex(c.double()),
                                            torch.view_as_complex(w.double())))
        _REF[case] = (c, w, {0: y, 1: y * _keep(L, M)})
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
@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_sfno_mix_vs_fp64(device, strict, case, tri):
    """Spectra that are truly zero where ``tri`` says so (the split table handed in, as the layers do)."""
    B, Cin, Cout, L, M = case
    c, w, refs = _case(case)
    f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", torch.ops.amd_dft.sfno_mix_info(B, Cin, Cout, L, M, 0))}
    assert (f["slabs"], f["otiles"], f["ogroups"], f["ctiles"]) == SHAPE[case] and f["coltile"] == 64
    cz = (c * _keep(L, M) if tri else c).to(device)
    wd = w.to(device)
    out = SP.sfno_mix(cz, wd, SP.sfno_mix_split(wd), tri)
    assert out.shape == (B, Cout, L, M, 2) and out.dtype == torch.float32
    err = _field_err(out, refs[tri])
    print(f"MEASURED sfno_mix {case} tri={tri} {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_sfno_mix_nonzero_where_l_below_m(device, strict, case, tri):
    """Random non-zero input where l < m (the op splits the weights itself here): ``tri = 0`` must use it;
    ``tri = 1`` must give the product of the zeroed spectrum, with exact 0.0 there."""
    B, Cin, Cout, L, M = case
    c, w, refs = _case(case)
    out = SP.sfno_mix(c.to(device), w.to(device), None, tri)
    err = _field_err(out, refs[tri])
    print(f"MEASURED sfno_mix dirty {case} tri={tri} {err:.3e}")
    assert err < TOL
    if tri == 0:
        assert _field_err(out, refs[1]) > 1e-2  # far from the zeroed product: nothing was skipped
    else:
        below = (~_keep(L, M))[None, None].expand(B, Cout, L, M, 2)
        assert torch.all(out.cpu()[below] == 0.0)


@pytest.mark.gpu
def test_sfno_mix_view_at_odd_offset(device, strict):
    """Input taken as a view at an odd float offset (the op copies it to an 8-byte boundary)."""
    case = CASES[1]
    c, w, refs = _case(case)
    buf = torch.zeros(c.numel() + 1, device=device)
    cv = buf[1:].view(c.shape)
    cv.copy_(c)
    assert cv.data_ptr() % 8 == 4
    wd = w.to(device)
    for tri in (0, 1):
        assert _field_err(SP.sfno_mix(cv, wd, SP.sfno_mix_split(wd), tri), refs[tri]) < TOL


@pytest.mark.gpu
def test_sfno_mix_split_on_device_and_argument_device(device, strict):
    """The device-built table equals the host-built one bit for bit; a table on another device is refused."""
    _, w, _ = _case(CASES[5])
    host = SP.sfno_mix_split(w)
    assert torch.equal(SP.sfno_mix_split(w.to(device)).cpu(), host)
    c = torch.zeros(1, 130, 12, 12, 2, device=device)
    with pytest.raises(RuntimeError, match="w_split"):
        torch.ops.amd_dft.sfno_mix(c, w.to(device), host, 0)


@pytest.mark.gpu
def test_sfno_mix_deterministic(device):
    c, w, _ = _case(CASES[4])
    cd, wd = c.to(device), w.to(device)
    ws = SP.sfno_mix_split(wd)
    for tri in (0, 1):
        assert torch.equal(SP.sfno_mix(cd, wd, ws, tri), SP.sfno_mix(cd, wd, ws, tri))


def _layer_input():
    g = torch.Generator().manual_seed(46)
    return torch.randn(1, 20, 46, 90, generator=g)


@pytest.mark.gpu
def test_layers_on_the_degree_kernel_vs_fp64(device, strict, monkeypatch):
    """``SphericalConv2d`` / ``SFNOBlock`` with the mix on ``sfno_mix``: through ``mix="auto"`` above the expansion
    bound (patched to 0) and through ``mix="degree"``.  The two routes differ from the expanded one only in the mix
    stage, whose own error the op-level bound covers: e_degree <= e_expanded + 1e-5, both against the fp64
    torch-backend reference."""
    torch.manual_seed(20)
    x = _layer_input()
    conv = SphericalConv2d(20, 20, 46, 90, backend="torch")
    blk = SFNOBlock(20, 46, 90, backend="torch")
    with torch.no_grad():
        ref_c = conv.double()(x.double())
        ref_b = blk.double()(x.double())
        conv, blk = conv.float().to(device).set_backend("amd"), blk.float().to(device).set_backend("amd")
        xd = x.to(device)
        assert conv.mix == "auto" and conv.expanded_bytes() <= sfno.EXPAND_LIMIT_BYTES
        e_c, e_b = _field_err(conv(xd), ref_c), _field_err(blk(xd), ref_b)  # the expanded route
        print(f"MEASURED sfno expanded conv {e_c:.3e} block {e_b:.3e}")

        def fail(*a):
            pytest.fail("the expanded route ran")

        monkeypatch.setattr(SP, "fno_spectral_mix", fail)
        monkeypatch.setattr(sfno, "EXPAND_LIMIT_BYTES", 0)
        a_c, a_b = _field_err(conv(xd), ref_c), _field_err(blk(xd), ref_b)  # "auto" above the bound
        monkeypatch.setattr(sfno, "EXPAND_LIMIT_BYTES", 256 << 20)
        conv.mix = blk.spectral.mix = "degree"
        d_c, d_b = _field_err(conv(xd), ref_c), _field_err(blk(xd), ref_b)
    print(f"MEASURED sfno auto-above-bound conv {a_c:.3e} block {a_b:.3e} degree conv {d_c:.3e} block {d_b:.3e}")
    assert a_c <= e_c + TOL and a_b <= e_b + TOL
    assert d_c <= e_c + TOL and d_b <= e_b + TOL


@pytest.mark.gpu
def test_degree_block_graph_capture(device, strict):
    torch.manual_seed(21)
    x = _layer_input().to(device)
    blk = SFNOBlock(20, 46, 90, backend="amd", mix="degree").to(device).eval()
    with torch.no_grad():
        eager = blk(x).clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = blk(x)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(y, eager)
