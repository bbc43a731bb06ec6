"""The transposed (upsampling) DISCO convolution, CPU tier: ``disco_transpose_tables``, ``disco_csr_transpose``, the
``disco_t`` op's ATen kernels, ``DiscreteContinuousConvTransposeS2``'s two backends, error checks, ``disco_t_info``
and export.  The gfx950 kernel: tests/test_disco_t_gpu.py.

The oracle is independent of the code under test: it evaluates the filter for every (input point, output point)
pair at their own longitudes from the formulas of the definition, as a dense [nlat_out, nlon_out, K, nlat_in, nlon_in]
fp64 tensor, normalises each output point by its own sum and contracts densely.  It assumes no longitude invariance
and never sees CSR."""
import math
import re

import numpy as np
import pytest
import torch

from tensorrt_dft_plugins_amd import load_plugins
from tensorrt_dft_plugins_amd.engine import Engine
from tensorrt_dft_plugins_amd.models import DiscreteContinuousConvS2, DiscreteContinuousConvTransposeS2
from tensorrt_dft_plugins_amd.onnx import exporter as ex
from tensorrt_dft_plugins_amd.onnx import proto as P
from tensorrt_dft_plugins_amd.onnx.runner import OnnxGraph
from tensorrt_dft_plugins_amd.ops import disco as D
from tensorrt_dft_plugins_amd.ops.sht import quadrature

load_plugins()
ops = torch.ops.amd_dft
BF = torch.bfloat16

# (in_shape (coarse), out_shape (fine), kernel_shape, grid_in, grid_out)
GRID_CASES = [
    ((9, 16), (17, 32), (3, 4), "equiangular", "equiangular"),
    ((6, 12), (12, 36), 2, "legendre-gauss", "legendre-gauss"),
    ((13, 24), (13, 24), 3, "equiangular", "equiangular"),
    ((6, 12), (13, 24), (2, 3), "legendre-gauss", "equiangular"),
]
IDS = ["eq9x16-s2-3x4", "lg6x12-s3-nr2", "eq13x24-s1-nr3", "lg-to-eq-s2-2x3"]


def _theta(n, grid):
    if grid == "equiangular":
        return np.pi * np.arange(n) / (n - 1)
    return np.arccos(np.polynomial.legendre.leggauss(n)[0][::-1])


def _oracle_psi(in_shape, out_shape, kernel_shape, grid_in, grid_out, normalize=True):
    """Dense PsiT [Ho, Wo, K, Hi, Wi] in fp64, brute force at every (output point, input point) pair."""
    (Hi, Wi), (Ho, Wo) = in_shape, out_shape
    nr, nphi = (kernel_shape, 0) if isinstance(kernel_shape, int) else kernel_shape
    K = nr if nphi == 0 else 1 + (nr - 1) * nphi
    cutoff = (nr + 1) * math.pi / (Hi - 1)
    dr = cutoff / nr
    thc, th = _theta(Hi, grid_in), _theta(Ho, grid_out)  # centres (input), evaluation points (output)
    q = quadrature(Hi, grid_in)[1] * 2.0 * math.pi / Wi
    psi = np.zeros((Ho, Wo, K, Hi, Wi))
    for k in range(Ho):
        for j in range(Wo):
            for kc in range(Hi):
                for jc in range(Wi):
                    phi = 2.0 * math.pi * j / Wo - 2.0 * math.pi * jc / Wi
                    z = math.cos(th[k]) * math.cos(thc[kc]) + math.sin(th[k]) * math.sin(thc[kc]) * math.cos(phi)
                    r = math.acos(min(1.0, max(-1.0, z)))
                    if r >= cutoff:
                        continue
                    X = math.cos(thc[kc]) * math.sin(th[k]) * math.cos(phi) - math.sin(thc[kc]) * math.cos(th[k])
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
                        psi[k, j, p, kc, jc] = v * q[kc]
    if normalize:
        total = psi.sum(axis=(2, 3, 4))
        psi /= np.where(total > 0.0, total, 1.0)[:, :, None, None, None]
    return psi


_CACHE = {}


def _case(i):
    """(oracle PsiT, z fp64 [2, 3, K, Hi, Wi], oracle y [2, 3, Ho, Wo], fp64 tables as tensors), built once."""
    if i not in _CACHE:
        ins, outs, ks, gi, go = GRID_CASES[i]
        psi = torch.from_numpy(_oracle_psi(ins, outs, ks, gi, go))
        g = torch.Generator().manual_seed(200 + i)
        z = torch.randn(2, 3, D.kernel_size(ks), *ins, dtype=torch.float64, generator=g)
        y = torch.einsum("kjpab,ncpab->nckj", psi, z)
        t64 = tuple(torch.from_numpy(a) for a in D.disco_transpose_tables(ins, outs, ks, gi, go, dtype=np.float64))
        _CACHE[i] = (psi, z, y, t64)
    return _CACHE[i]


def _op(z, tables, case, bias=None):
    return ops.disco_t(z, *tables, case[1][0], case[1][1], bias)


@pytest.mark.parametrize("i", range(len(GRID_CASES)), ids=IDS)
def test_cpu_op_and_torch_backend_against_the_brute_force_oracle(i):
    case = GRID_CASES[i]
    ins, outs, ks, gi, go = case
    _, z, y, t64 = _case(i)
    got = _op(z, t64, case)
    assert got.dtype == torch.float64 and got.shape == y.shape
    err = (got - y).abs().max().item()
    m = DiscreteContinuousConvTransposeS2(4, 3, ins, outs, ks, grid_in=gi, grid_out=go, backend="torch")
    errt = (m.gather_torch(z) - y).abs().max().item()
    print(f"MEASURED disco_t oracle {IDS[i]} cpu op {err:.3e} torch backend {errt:.3e}")
    assert err < 1e-12 and errt < 1e-12
    # the whole module, torch backend in fp64, against the contraction written out
    with torch.no_grad():
        m.bias.normal_()
        x = torch.randn(2, 4, *ins, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
        zz = torch.einsum("ocp,ncab->nopab", m.weight.double(), x)
        ref = torch.einsum("kjpab,nopab->nokj", _case(i)[0], zz) + m.bias.double()[None, :, None, None]
        assert (m(x) - ref).abs().max().item() < 1e-12


@pytest.mark.parametrize("i", range(len(GRID_CASES)), ids=IDS)
def test_tables_layout(i):
    ins, outs, ks, gi, go = GRID_CASES[i]
    rp, idx, val = D.disco_transpose_tables(ins, outs, ks, gi, go)
    K = D.kernel_size(ks)
    s = outs[1] // ins[1]
    cols = K * ins[0] * ins[1]
    assert rp.dtype == np.int32 and idx.dtype == np.int32 and val.dtype == np.float32
    assert rp.shape == (outs[0] * s + 1,) and rp[0] == 0 and rp[-1] == len(idx) == len(val)
    assert (np.diff(rp) > 0).all() and (val > 0).all() and idx.min() >= 0 and idx.max() < cols
    for r in range(outs[0] * s):
        assert (np.diff(idx[rp[r]:rp[r + 1]]) > 0).all()  # sorted, no duplicates
    # the stored entries are exactly the oracle's non-zeros at t = 0: output longitudes rho = 0 .. s - 1, columns
    # k'-major (k', p, d)
    psi = _case(i)[0]
    v64 = D.disco_transpose_tables(ins, outs, ks, gi, go, dtype=np.float64)[2]
    dense = np.zeros((outs[0] * s, cols))
    dense[np.repeat(np.arange(outs[0] * s), np.diff(rp)), idx] = v64
    want = psi[:, :s].permute(0, 1, 3, 2, 4).reshape(outs[0] * s, cols).numpy()
    # (an angular hat that one side rounds to 0 and the other to 1e-17 is inside the bound, as in test_disco.py)
    assert np.abs(dense - want).max() < 1e-14
    assert ((dense > 1e-14) <= (want > 0)).all() and ((want > 1e-14) <= (dense > 0)).all()


@pytest.mark.parametrize("i", range(len(GRID_CASES)), ids=IDS)
def test_constant_field_gives_one(i):
    """z = 1 gives y = 1.  The brute-force oracle itself deviates from 1 by a few 1e-16 on these grids (each output
    point is a normalised sum of up to a few hundred positive terms).  The op sums the same values in another order,
    so it gets the oracle's deviation plus one fp64 rounding per entry of an output point."""
    case = GRID_CASES[i]
    psi, _, _, t64 = _case(i)
    dev = (psi.sum(dim=(2, 3, 4)) - 1.0).abs().max().item()
    n_e = int((psi > 0).sum(dim=(2, 3, 4)).max())
    one = torch.ones(1, 1, D.kernel_size(case[2]), *case[0], dtype=torch.float64)
    got = (_op(one, t64, case) - 1.0).abs().max().item()
    print(f"MEASURED disco_t constant {IDS[i]} oracle deviation {dev:.3e} op {got:.3e} entries {n_e}")
    assert got <= dev + n_e * 2.0 ** -53


@pytest.mark.parametrize("i", range(len(GRID_CASES)), ids=IDS)
def test_longitude_roll(i):
    case = GRID_CASES[i]
    s = case[1][1] // case[0][1]
    _, z, y, t64 = _case(i)
    for t in (1, 5):
        assert torch.equal(_op(torch.roll(z, t, dims=-1), t64, case), torch.roll(_op(z, t64, case), s * t, dims=-1))
        assert (_op(torch.roll(z, t, dims=-1), t64, case) - torch.roll(y, s * t, dims=-1)).abs().max() < 1e-12


@pytest.mark.parametrize("i", range(len(GRID_CASES)), ids=IDS)
def test_csr_transpose_is_the_adjoint_of_the_forward_table(i):
    """<disco(x), z> = <x, disco_t(z)> for the re-indexed table of an arbitrary forward table (here the normalised
    forward table from the fine grid to the coarse one), in fp64 to 1e-12 relative."""
    coarse, fine, ks, gc, gf = GRID_CASES[i]
    K = D.kernel_size(ks)
    fwd = D.disco_tables(fine, coarse, ks, gf, gc, dtype=np.float64)
    tr = D.disco_csr_transpose(*fwd, K, fine, coarse)
    s = fine[1] // coarse[1]
    assert tr[0].dtype == np.int32 and tr[1].dtype == np.int32 and tr[2].dtype == np.float64
    assert tr[0].shape == (fine[0] * s + 1,) and len(tr[1]) == len(fwd[1])
    assert np.array_equal(np.sort(tr[2]), np.sort(fwd[2]))  # a permutation: no reweighting
    g = torch.Generator().manual_seed(300 + i)
    x = torch.randn(3, *fine, dtype=torch.float64, generator=g)
    z = torch.randn(3, K, *coarse, dtype=torch.float64, generator=g)
    lhs = (ops.disco(x, *(torch.from_numpy(a) for a in fwd), K, *coarse) * z).sum().item()
    rhs = (x * ops.disco_t(z[None], *(torch.from_numpy(a) for a in tr), *fine)[0]).sum().item()
    print(f"MEASURED disco_t adjoint {IDS[i]} {lhs:.15e} {rhs:.15e}")
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def test_cpu_op_fp32_bf16_out_and_meta():
    case = GRID_CASES[0]
    ins, outs, ks, gi, go = case
    K = D.kernel_size(ks)
    _, z, y, _ = _case(0)
    t = tuple(torch.from_numpy(a) for a in D.disco_transpose_tables(ins, outs, ks, gi, go))
    o32 = _op(z.float(), t, case)
    assert o32.dtype == torch.float32 and (o32.double() - y).abs().max() < 1e-6
    ob = _op(z.to(BF), t, case)
    ref = _op(z.to(BF).double(), tuple(a.double() if a.is_floating_point() else a for a in t), case)
    assert ob.dtype == BF and (ob.double() - ref).abs().max() <= 2.0 ** -8 * ref.abs().max()
    bias = torch.randn(3)
    for zz in (z.float(), z.to(BF)):
        want = _op(zz, t, case, bias)
        out = torch.empty_like(want)
        assert ops.disco_t_out(zz, *t, *outs, bias, out) is out and torch.equal(out, want)
    with torch.device("meta"):
        ym = ops.disco_t(torch.empty(5, 2, K, *ins), torch.empty(1, dtype=torch.int32),
                         torch.empty(1, dtype=torch.int32), torch.empty(1), *outs)
    assert ym.shape == (5, 2, *outs) and ym.device.type == "meta"
    zf = z.float()
    for out in (torch.empty(2, 3, outs[0], outs[1] + 1), torch.empty(2, 3, *outs, dtype=BF),
                torch.empty(2, 3, outs[1], outs[0]).transpose(-1, -2), torch.empty(2, 3, *outs, device="meta")):
        with pytest.raises(RuntimeError, match="disco_t_out: "):
            ops.disco_t_out(zf, *t, *outs, None, out)


def test_bias_per_channel_over_leading_batch_dimensions():
    case = GRID_CASES[3]
    ins, outs, ks, gi, go = case
    K = D.kernel_size(ks)
    t64 = _case(3)[3]
    g = torch.Generator().manual_seed(9)
    z = torch.randn(2, 3, 5, K, *ins, dtype=torch.float64, generator=g)
    bias = torch.randn(5, dtype=torch.float64, generator=g)
    plain = _op(z, t64, case)
    got = _op(z, t64, case, bias)
    assert got.shape == (2, 3, 5, *outs)
    assert torch.equal(got, plain + bias[None, None, :, None, None])
    # fp32: the bias joins the fp64 sum before the one rounding
    t32 = tuple(a.float() if a.is_floating_point() else a for a in t64)
    want = (_op(z.float().double(), (t32[0], t32[1], t32[2].double()), case)
            + bias.float().double()[None, None, :, None, None]).float()
    assert torch.equal(_op(z.float(), t32, case, bias.float()), want)


def test_module_amd_backend_on_cpu_tensors():
    ins, outs, ks, gi, go = GRID_CASES[0]
    torch.manual_seed(2)
    m = DiscreteContinuousConvTransposeS2(3, 5, ins, outs, ks, grid_in=gi, grid_out=go).eval()
    assert m.theta_cutoff == D.default_cutoff(ks, ins[0])  # the coarse grid sets the footprint
    with torch.no_grad():
        m.bias.normal_()
        x = torch.randn(2, 3, *ins, dtype=torch.float64)
        ref = m.set_backend("torch")(x)
        got = m.set_backend("amd")(x.float())
        gotb = m(x.to(BF))
    assert ref.dtype == torch.float64
    assert got.shape == (2, 5, *outs) and got.dtype == torch.float32
    assert ((got.double() - ref).norm() / ref.norm()).item() < 1e-5
    assert gotb.dtype == BF and ((gotb.double() - ref).norm() / ref.norm()).item() < 2e-2
    assert m.set_backend("torch")(x.to(BF)).dtype == BF
    nb = DiscreteContinuousConvTransposeS2(3, 5, ins, outs, ks, bias=False)
    assert nb.bias is None and nb(x.float()).shape == (2, 5, *outs)
    t = m.tables("cpu")
    assert (t.K, t.s, t.nnz) == (D.kernel_size(ks), 2, len(t.idx)) and t.nnz_max == int(np.diff(t.row_ptr_host).max())
    assert m.tables("cpu") is t and "in_shape=(9, 16)" in repr(m) and "backend='torch'" in repr(m)


def test_errors_before_any_launch():
    with pytest.raises(ValueError):
        D.disco_transpose_tables((13, 9), (13, 24), 3)
    with pytest.raises(ValueError):
        D.disco_transpose_tables((13, 24), (13, 24), 3, grid_in="lobatto")
    with pytest.raises(ValueError):
        D.disco_transpose_tables((13, 24), (13, 24), (3, 0))
    with pytest.raises(TypeError):
        D.disco_transpose_tables((13, 24), (13, 24), 3, dtype=np.float16)
    with pytest.raises(OverflowError):
        D.disco_transpose_tables((2 ** 16, 2 ** 14), (2 ** 16, 2 ** 14), 2)
    with pytest.raises(ValueError):
        D.disco_csr_transpose(np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0), 3, (13, 25), (13, 24))
    with pytest.raises(ValueError):
        DiscreteContinuousConvTransposeS2(2, 2, (7, 10), (13, 24), 3)
    with pytest.raises(ValueError):
        DiscreteContinuousConvTransposeS2(2, 2, (13, 24), (13, 24), 3, backend="cuda")
    m = DiscreteContinuousConvTransposeS2(2, 2, (13, 24), (13, 24), 3)
    with pytest.raises(ValueError):
        m.set_backend("cuda")
    with pytest.raises(ValueError):
        m(torch.randn(1, 2, 13, 25))
    with pytest.raises(TypeError):
        m(torch.randn(1, 2, 13, 24, dtype=torch.float64))
    with pytest.raises(TypeError):
        D.disco_transpose(torch.randn(1, 2, 3, 13, 24, dtype=torch.float64), m.tables("cpu"))
    rp, idx, val = (torch.from_numpy(a) for a in D.disco_transpose_tables((13, 24), (13, 24), 3))
    z = torch.randn(2, 2, 3, 13, 24)
    b = torch.randn(2)
    ops.disco_t(z, rp, idx, val, 13, 24, b)
    for bad in ((z.to(torch.float16), rp, idx, val), (z, rp.long(), idx, val), (z, rp, idx.long(), val),
                (z, rp, idx, val.double()), (z.double(), rp, idx, val), (z, rp, idx, val.to(BF)),
                (z, rp[:-1], idx, val), (z, rp, idx[:-1], val), (z[0, 0], rp, idx, val)):
        with pytest.raises(RuntimeError):
            ops.disco_t(*bad, 13, 24)
    for bad_bias in (torch.randn(3), b.double(), b.to(BF), torch.randn(2, 1)):
        with pytest.raises(RuntimeError, match="bias"):
            ops.disco_t(z, rp, idx, val, 13, 24, bad_bias)
    with pytest.raises(RuntimeError, match="multiple"):
        ops.disco_t(z, rp, idx, val, 13, 36)
    dec = rp.clone()
    dec[5] = dec[4] - 1
    with pytest.raises(RuntimeError, match="decrease"):
        ops.disco_t(z, dec, idx, val, 13, 24)
    far = idx.clone()
    far[7] = 3 * 13 * 24
    with pytest.raises(RuntimeError, match="outside"):
        ops.disco_t(z, rp, far, val, 13, 24)


def test_disco_t_info_on_the_host():
    def fields(*a):
        return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", ops.disco_t_info(*a))}

    f = fields(20, 360, 720, 3, 720, 1440, 1000, False)  # an LDS row is 3 * 720 * 4 bytes: 7 of them fit
    assert f["PT"] == 1 and f["rows"] == 7 and f["lds"] == 7 * 3 * 720 * 4 and f["wgs"] == 720 * 20
    assert f["passes"] == 1 and f["phases"] == 2 and f["items"] == 3 and f["threads"] == 256 and "bf16" not in f
    f = fields(64, 180, 360, 9, 180, 360, 1000, True)
    assert f["PT"] == 1 and f["rows"] == 5 and f["wgs"] == 180 * 64 and f["phases"] == 1 and f["bf16"] == 1
    f = fields(5, 9, 16, 9, 17, 32, 1000, False)
    assert f["PT"] == 4 and f["rows"] == 9 and f["lds"] == 4 * 9 * 9 * 16 * 4 and f["ptiles"] == 2 and f["wgs"] == 34
    f = fields(5, 9, 200, 2, 9, 200, 1000, False)
    assert f["PT"] == 4 and f["passes"] == 2 and f["rows"] == 9
    assert "PT=1" in ops.disco_t_info(3, 13, 24, 3, 13, 24, 10, False)  # fewer than four planes
    for bad in ((0, 13, 24, 3, 13, 24, 10), (1, 13, 24, 3, 13, 36, 10), (1, 13, 24, 3, 13, 24, -1),
                (1, 2, 8192, 3, 2, 8192, 10), (1, 13, 24, 0, 13, 24, 10)):
        with pytest.raises(RuntimeError):
            ops.disco_t_info(*bad, False)


def test_export_runner_engine_encoder_decoder(tmp_path):
    coarse, fine, ks, gc, gf = GRID_CASES[0]
    torch.manual_seed(4)
    m = torch.nn.Sequential(
        DiscreteContinuousConvS2(3, 4, fine, coarse, ks, grid_in=gf, grid_out=gc),
        DiscreteContinuousConvTransposeS2(4, 3, coarse, fine, ks, grid_in=gc, grid_out=gf)).eval()
    x = torch.randn(2, 3, *fine)
    with torch.no_grad():
        m[1].bias.normal_()
        eager = m(x)
    assert eager.shape == x.shape
    data = ex.export(m, (x,))
    nodes = P.load_model(data).graph.node
    assert [n.op_type for n in nodes if n.domain == "com.amd.dft"] == ["disco", "fno_pointwise", "fno_pointwise",
                                                                       "disco_t"]
    stock = {n.op_type for n in nodes if n.domain != "com.amd.dft"}
    print(f"MEASURED disco_t export other nodes {sorted(stock)}")
    assert stock <= {"Constant", "Reshape"}
    (y,) = OnnxGraph(data, torch.device("cpu")).run(x)
    assert torch.equal(y, eager)
    eng = Engine.build(m, (x,), device="cpu")
    (ye,) = eng.infer(x)
    assert torch.equal(ye, eager)
    path = str(tmp_path / "disco_t.engine")
    eng.save(path)
    (yl,) = Engine.load(path, device="cpu").infer(x)
    assert torch.equal(yl, eager)


def test_reexports_and_the_deny_list():
    import tensorrt_dft_plugins_amd as tdp
    from tensorrt_dft_plugins_amd import models
    from tensorrt_dft_plugins_amd.onnx.runner import _AMD_NODE_DENY

    assert tdp.disco_transpose is D.disco_transpose and tdp.disco_transpose_tables is D.disco_transpose_tables
    assert models.DiscreteContinuousConvTransposeS2 is DiscreteContinuousConvTransposeS2
    assert "disco_t_out" in _AMD_NODE_DENY and "disco_t" not in _AMD_NODE_DENY
