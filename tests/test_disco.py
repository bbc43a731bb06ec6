"""DISCO convolutions on the sphere, CPU tier: ``disco_tables``, the ``disco`` op's ATen kernels, the module's two
backends, error checks, ``disco_info`` and export.  The gfx950 kernel: tests/test_disco_gpu.py.

The oracle is independent of the code under test: it evaluates the filter for every output point at its own
longitude phi' = 2 pi j' / nlon_out from the formulas of the definition with phi - phi', as a dense
[K, nlat_out, nlon_out, nlat_in, nlon_in] fp64 tensor, normalises each output point by its own sum and contracts
densely.  It assumes no longitude invariance and never sees CSR."""
import math
import re

import numpy as np
import pytest
import torch

from tensorrt_dft_plugins_amd import load_plugins
from tensorrt_dft_plugins_amd.engine import Engine
from tensorrt_dft_plugins_amd.models import DiscreteContinuousConvS2
from tensorrt_dft_plugins_amd.onnx import exporter as ex
from tensorrt_dft_plugins_amd.onnx import proto as P
from tensorrt_dft_plugins_amd.onnx.runner import OnnxGraph
from tensorrt_dft_plugins_amd.ops import disco as D
from tensorrt_dft_plugins_amd.ops.sht import quadrature

load_plugins()
ops = torch.ops.amd_dft
BF = torch.bfloat16

# (in_shape, out_shape, kernel_shape, grid_in, grid_out)
GRID_CASES = [
    ((13, 24), (13, 24), 3, "equiangular", "equiangular"),
    ((17, 32), (9, 16), (3, 4), "equiangular", "equiangular"),
    ((12, 36), (6, 12), 2, "legendre-gauss", "legendre-gauss"),
    ((13, 24), (6, 12), (2, 3), "equiangular", "legendre-gauss"),
]
IDS = ["eq13x24-s1-nr3", "eq17x32-s2-3x4", "lg12x36-s3-nr2", "eq-to-lg-s2-2x3"]


def _theta(n, grid):
    if grid == "equiangular":
        return np.pi * np.arange(n) / (n - 1)
    return np.arccos(np.polynomial.legendre.leggauss(n)[0][::-1])


def _oracle_psi(in_shape, out_shape, kernel_shape, grid_in, grid_out, normalize=True):
    """Dense Psi [K, Ho, Wo, Hi, Wi] in fp64, brute force at every output point."""
    (Hi, Wi), (Ho, Wo) = in_shape, out_shape
    nr, nphi = (kernel_shape, 0) if isinstance(kernel_shape, int) else kernel_shape
    K = nr if nphi == 0 else 1 + (nr - 1) * nphi
    cutoff = (nr + 1) * math.pi / (Ho - 1)
    dr = cutoff / nr
    th, thp = _theta(Hi, grid_in), _theta(Ho, grid_out)
    q = quadrature(Hi, grid_in)[1] * 2.0 * math.pi / Wi
    psi = np.zeros((K, Ho, Wo, Hi, Wi))
    for kp in range(Ho):
        for jp in range(Wo):
            for k in range(Hi):
                for j in range(Wi):
                    phi = 2.0 * math.pi * j / Wi - 2.0 * math.pi * jp / Wo
                    z = math.cos(th[k]) * math.cos(thp[kp]) + math.sin(th[k]) * math.sin(thp[kp]) * math.cos(phi)
                    r = math.acos(min(1.0, max(-1.0, z)))
                    if r >= cutoff:
                        continue
                    X = math.cos(thp[kp]) * math.sin(th[k]) * math.cos(phi) - math.sin(thp[kp]) * math.cos(th[k])
                    Y = math.sin(th[k]) * math.sin(phi)
                    g = math.atan2(Y, X) % (2.0 * math.pi)
                    hat = [max(0.0, 1.0 - abs(r - i * dr) / dr) for i in range(nr)]
                    if nphi == 0:
                        vals = hat
                    else:
                        vals = [hat[0]]
                        for i in range(1, nr):
                            for a in range(nphi):
                                d = abs(g - 2.0 * math.pi * a / nphi)
                                d = min(d, 2.0 * math.pi - d)
                                vals.append(hat[i] * max(0.0, 1.0 - d / (2.0 * math.pi / nphi)))
                    for p, v in enumerate(vals):
                        psi[p, kp, jp, k, j] = v * q[k]
    if normalize:
        psi /= psi.sum(axis=(0, 3, 4))[None, :, :, None, None]
    return psi


_CACHE = {}


def _case(i):
    """(oracle Psi, x fp64 [2, 3, Hi, Wi], oracle y [2, 3, K, Ho, Wo], fp64 tables as tensors), built once."""
    if i not in _CACHE:
        ins, outs, ks, gi, go = GRID_CASES[i]
        psi = torch.from_numpy(_oracle_psi(ins, outs, ks, gi, go))
        g = torch.Generator().manual_seed(100 + i)
        x = torch.randn(2, 3, *ins, dtype=torch.float64, generator=g)
        y = torch.einsum("pkjab,ncab->ncpkj", psi, x)
        t64 = tuple(torch.from_numpy(a) for a in D.disco_tables(ins, outs, ks, gi, go, dtype=np.float64))
        _CACHE[i] = (psi, x, y, t64)
    return _CACHE[i]


def _op(x, tables, case):
    _, outs, ks, _, _ = case
    return ops.disco(x, *tables, D.kernel_size(ks), outs[0], outs[1])


@pytest.mark.parametrize("i", range(len(GRID_CASES)), ids=IDS)
def test_cpu_op_and_torch_backend_against_the_brute_force_oracle(i):
    case = GRID_CASES[i]
    ins, outs, ks, gi, go = case
    _, x, y, t64 = _case(i)
    got = _op(x, t64, case)
    assert got.dtype == torch.float64 and got.shape == y.shape
    err = (got - y).abs().max().item()
    m = DiscreteContinuousConvS2(3, 4, ins, outs, ks, grid_in=gi, grid_out=go, backend="torch")
    errt = (m.gather_torch(x) - y).abs().max().item()
    print(f"MEASURED disco oracle {IDS[i]} cpu op {err:.3e} torch backend {errt:.3e}")
    assert err < 1e-12 and errt < 1e-12
    # the whole module, torch backend in fp64, against the contraction written out
    with torch.no_grad():
        ref = torch.einsum("ocp,ncpkj->nokj", m.weight.double(), y) + m.bias.double()[None, :, None, None]
        assert (m(x) - ref).abs().max().item() < 1e-12


@pytest.mark.parametrize("i", range(len(GRID_CASES)), ids=IDS)
def test_tables_layout(i):
    ins, outs, ks, gi, go = GRID_CASES[i]
    rp, idx, val = D.disco_tables(ins, outs, ks, gi, go)
    K = D.kernel_size(ks)
    assert rp.dtype == np.int32 and idx.dtype == np.int32 and val.dtype == np.float32
    assert rp.shape == (K * outs[0] + 1,) and rp[0] == 0 and rp[-1] == len(idx) == len(val)
    assert (np.diff(rp) >= 0).all() and (val > 0).all() and idx.min() >= 0 and idx.max() < ins[0] * ins[1]
    for r in range(K * outs[0]):
        assert (np.diff(idx[rp[r]:rp[r + 1]]) > 0).all()  # sorted, no duplicates
    # the stored entries are exactly the oracle's non-zeros at j' = 0
    psi = _case(i)[0]
    dense = np.zeros((K * outs[0], ins[0] * ins[1]))
    dense[np.repeat(np.arange(K * outs[0]), np.diff(rp)), idx] = D.disco_tables(ins, outs, ks, gi, go, dtype=np.float64)[2]
    assert np.abs(dense - psi[:, :, 0].reshape(K * outs[0], -1).numpy()).max() < 1e-14


@pytest.mark.parametrize("i", range(len(GRID_CASES)), ids=IDS)
def test_constant_field_sums_to_one(i):
    """sum_p y_p = 1 for a constant field.  The brute-force oracle itself deviates from 1 by at most 4.5e-16 on these
    grids (measured; each output point is a normalised sum of up to 791 positive terms).  The op sums the same
    values in another order, so it gets the oracle's deviation plus one fp64 rounding per entry of an output
    point."""
    case = GRID_CASES[i]
    psi, _, _, t64 = _case(i)
    dev = (psi.sum(dim=(0, 3, 4)) - 1.0).abs().max().item()
    n_e = int((psi > 0).sum(dim=(0, 3, 4)).max())
    one = torch.ones(1, 1, *case[0], dtype=torch.float64)
    got = (_op(one, t64, case).sum(dim=2) - 1.0).abs().max().item()
    print(f"MEASURED disco constant {IDS[i]} oracle deviation {dev:.3e} op {got:.3e} entries {n_e}")
    assert got <= dev + n_e * 2.0 ** -53


@pytest.mark.parametrize("i", range(len(GRID_CASES)), ids=IDS)
def test_longitude_roll(i):
    case = GRID_CASES[i]
    s = case[0][1] // case[1][1]
    _, x, y, t64 = _case(i)
    for t in (1, 5):
        assert torch.equal(_op(torch.roll(x, s * t, dims=-1), t64, case), torch.roll(_op(x, t64, case), t, dims=-1))
        assert (_op(torch.roll(x, s * t, dims=-1), t64, case) - torch.roll(y, t, dims=-1)).abs().max() < 1e-12


def test_isotropic_equiangular_commutes_with_the_flip():
    """Bound: the definition takes r = arccos(z).  Where an input point coincides with the output point (s = 1, the
    same grid) z = 1 up to a few fp64 roundings, and arccos turns an error e of z into sqrt(2 e) of r: with four
    roundings, sqrt(8 * 2^-52) = 4.2e-8 instead of 0, on one side of the equator and not on the other, since
    cos(pi - theta) and -cos(theta) round differently.  That entry's psi moves by 4.2e-8 / dr; it enters the
    result once with a normalised weight <= 1 and once through the normalisation, so |difference| <=
    2 * 4.2e-8 / dr * max|x|.  Every other entry is conditioned like 2^-52 / sin(r).  Measured 3.5e-9."""
    case = GRID_CASES[0]
    _, x, _, t64 = _case(0)
    a = _op(torch.flip(x, dims=(-2,)), t64, case)
    b = torch.flip(_op(x, t64, case), dims=(-2,))
    dr = D.default_cutoff(3, 13) / 3
    err = (a - b).abs().max().item()
    print(f"MEASURED disco flip {err:.3e}")
    assert err <= 2.0 * math.sqrt(8.0 * 2.0 ** -52) / dr * x.abs().max().item()


@pytest.mark.parametrize("ks", [3, (3, 4), (4, 5), 1])
def test_basis_partition_of_unity(ks):
    nr, nphi = D._kernel_shape(ks)
    cutoff = 0.37
    dr = cutoff / nr
    g = np.random.default_rng(3)
    r = np.concatenate([g.uniform(0.0, cutoff * 1.5, 4000), [0.0, (nr - 1) * dr, cutoff]])
    gamma = g.uniform(0.0, 2.0 * np.pi, r.shape)
    psis = D._basis(r, gamma, nr, nphi, cutoff)
    assert len(psis) == D.kernel_size(ks)
    total = np.sum(psis, axis=0)
    inside, outside = r <= (nr - 1) * dr, r >= cutoff
    assert np.abs(total[inside] - 1.0).max() < 1e-13 if inside.any() else True
    assert (total[outside] == 0.0).all() and all((p >= 0.0).all() for p in psis)


def test_cpu_op_fp32_and_bf16():
    case = GRID_CASES[1]
    ins, outs, ks, gi, go = case
    _, x, y, _ = _case(1)
    t = tuple(torch.from_numpy(a) for a in D.disco_tables(ins, outs, ks, gi, go))
    o32 = _op(x.float(), t, case)
    assert o32.dtype == torch.float32 and (o32.double() - y).abs().max() < 1e-6
    ob = _op(x.to(BF), t, case)
    ref = _op(x.to(BF).double(), tuple(a.double() if a.is_floating_point() else a for a in t), case)
    assert ob.dtype == BF and (ob.double() - ref).abs().max() <= 2.0 ** -8 * ref.abs().max()
    out = torch.empty_like(o32)
    assert ops.disco_out(x.float(), *t, D.kernel_size(ks), *outs, out) is out and torch.equal(out, o32)
    with torch.device("meta"):
        ym = ops.disco(torch.empty(5, *ins), torch.empty(1, dtype=torch.int32), torch.empty(1, dtype=torch.int32),
                       torch.empty(1), 9, *outs)
    assert ym.shape == (5, 9, *outs)


def test_module_amd_backend_on_cpu_tensors():
    ins, outs, ks, gi, go = GRID_CASES[1]
    torch.manual_seed(2)
    m = DiscreteContinuousConvS2(3, 5, ins, outs, ks, grid_in=gi, grid_out=go).eval()
    with torch.no_grad():
        m.bias.normal_()
        x = _case(1)[1]
        ref = m.set_backend("torch")(x)
        got = m.set_backend("amd")(x.float())
    assert got.shape == (2, 5, *outs) and got.dtype == torch.float32
    assert ((got.double() - ref).norm() / ref.norm()).item() < 1e-5


def test_errors_before_any_launch():
    with pytest.raises(ValueError):
        D.disco_tables((13, 24), (13, 9), 3)
    with pytest.raises(ValueError):
        D.disco_tables((13, 24), (13, 24), 3, grid_in="lobatto")
    with pytest.raises(ValueError):
        DiscreteContinuousConvS2(2, 2, (13, 24), (7, 10), 3)
    with pytest.raises(ValueError):
        DiscreteContinuousConvS2(2, 2, (13, 24), (13, 24), 3, backend="cuda")
    case = GRID_CASES[0]
    rp, idx, val = (torch.from_numpy(a) for a in D.disco_tables(*case))
    x = torch.randn(2, 13, 24)
    ops.disco(x, rp, idx, val, 3, 13, 24)
    for bad in ((x.to(torch.float16), rp, idx, val), (x, rp.long(), idx, val), (x, rp, idx.long(), val),
                (x, rp, idx, val.double()), (x.double(), rp, idx, val), (x, rp, idx, val.to(BF)),
                (x, rp[:-1], idx, val), (x, rp, idx[:-1], val), (x[0, 0], rp, idx, val)):
        with pytest.raises(RuntimeError):
            ops.disco(*bad, 3, 13, 24)
    with pytest.raises(RuntimeError, match="multiple"):
        ops.disco(x, rp, idx, val, 3, 13, 9)
    dec = rp.clone()
    dec[5] = dec[4] - 1
    with pytest.raises(RuntimeError, match="decrease"):
        ops.disco(x, dec, idx, val, 3, 13, 24)
    far = idx.clone()
    far[7] = 13 * 24
    with pytest.raises(RuntimeError, match="outside"):
        ops.disco(x, rp, far, val, 3, 13, 24)
    for out in (torch.empty(2, 3, 13, 25), torch.empty(2, 3, 13, 24, dtype=BF),
                torch.empty(2, 3, 24, 13).transpose(-1, -2)):
        with pytest.raises(RuntimeError):
            ops.disco_out(x, rp, idx, val, 3, 13, 24, out)


def test_disco_info_on_the_host():
    f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", ops.disco_info(64, 180, 360, 9, 180, 360, 1000, False))}
    assert f["PT"] == 4 and f["rows"] == 11 and f["lds"] == 4 * 11 * 360 * 4 and f["wgs"] == 180 * 16
    assert f["passes"] == 2 and f["items"] == 3 and f["threads"] == 256
    f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", ops.disco_info(20, 720, 1440, 3, 360, 720, 1000, True))}
    assert f["PT"] == 1 and f["rows"] == 11 and f["wgs"] == 360 * 20 and f["passes"] == 1 and f["bf16"] == 1
    assert "PT=1" in ops.disco_info(3, 13, 24, 3, 13, 24, 10, False)  # fewer than four planes
    for bad in ((0, 13, 24, 3, 13, 24, 10), (1, 13, 24, 3, 13, 9, 10), (1, 13, 24, 3, 13, 24, -1),
                (1, 2, 32768, 3, 2, 32768, 10)):
        with pytest.raises(RuntimeError):
            ops.disco_info(*bad, False)


def test_export_runner_engine(tmp_path):
    ins, outs, ks, gi, go = GRID_CASES[1]
    torch.manual_seed(4)
    m = DiscreteContinuousConvS2(3, 5, ins, outs, ks, grid_in=gi, grid_out=go).eval()
    x = torch.randn(2, 3, *ins)
    with torch.no_grad():
        eager = m(x)
    data = ex.export(m, (x,))
    nodes = P.load_model(data).graph.node
    assert [n.op_type for n in nodes if n.domain == "com.amd.dft"] == ["disco", "fno_pointwise"]
    # every compute node is a com.amd.dft op: what is left in the default domain holds constants or is the view
    stock = {n.op_type for n in nodes if n.domain != "com.amd.dft"}
    print(f"MEASURED disco export other nodes {sorted(stock)}")
    assert stock <= {"Constant", "Reshape"}
    (y,) = OnnxGraph(data, torch.device("cpu")).run(x)
    assert torch.equal(y, eager)
    eng = Engine.build(m, (x,), device="cpu")
    (ye,) = eng.infer(x)
    assert torch.equal(ye, eager)
    path = str(tmp_path / "disco.engine")
    eng.save(path)
    (yl,) = Engine.load(path, device="cpu").infer(x)
    assert torch.equal(yl, eager)


def test_reexports():
    import tensorrt_dft_plugins_amd as tdp

    assert tdp.disco is D.disco and tdp.disco_tables is D.disco_tables
    from tensorrt_dft_plugins_amd.onnx.runner import _AMD_NODE_DENY

    assert "disco_out" in _AMD_NODE_DENY and "disco" not in _AMD_NODE_DENY
