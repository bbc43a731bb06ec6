"""The longitude-Fourier DISCO route on the CPU: the packed tables against the dense fp64 formulas, the CPU op with
``numpy.fft`` around it against the fp64 definition, and the module with ``algorithm="spectral"`` through ONNX.
The six shapes: s = 1, 2, 3; nlon_out even and odd; G real and complex; R = 8, 4 and 1 (K = 9); bands clipped at both
poles; ragged last groups (``s1``, ``s3``, ``odd``: nlat_out = 9, 7, 5 against R = 8, 4, 4)."""
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

load_plugins()
ops = torch.ops.amd_dft

# name -> (in_shape, out_shape, kernel_shape, grid)
SHAPES = {
    "s1": ((9, 16), (9, 16), 2, "equiangular"),
    "k9": ((17, 32), (9, 16), (3, 4), "equiangular"),
    "s3": ((12, 30), (7, 10), 3, "equiangular"),
    "odd": ((9, 15), (5, 5), (2, 3), "equiangular"),
    "lg": ((8, 14), (8, 7), 2, "legendre-gauss"),
    "m17": ((33, 64), (17, 32), (3, 4), "equiangular"),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_tables_against_the_dense_formula(name):
    ins, outs, ks, grid = SHAPES[name]
    (Hi, Wi), (Ho, Wo) = ins, outs
    K, s, Mo = D.kernel_size(ks), Wi // Wo, Wo // 2 + 1
    rp, idx, val = D.disco_tables(ins, outs, ks, grid, grid, dtype=np.float64)
    psi = np.zeros((K * Ho, Hi * Wi))
    psi[np.repeat(np.arange(K * Ho), np.diff(rp)), idx] = val
    psi = psi.reshape(K, Ho, Hi, Wi)
    Gf = np.conj(np.fft.fft(psi, axis=-1))  # G[p, k', k, mu], the full spectrum
    T, lo, U = D.disco_spectral_tables(ins, outs, ks, grid, grid, dtype=np.float64)
    R = D.disco_spectral_group(K)
    assert T.shape == (-(-Ho // R), Mo, 16, -(-2 * s * U // 32) * 32) and lo.dtype == np.int32
    want = np.zeros_like(T)
    touched = np.abs(psi).sum(axis=(0, 3)) > 0  # [k', k]
    for kp in range(Ho):
        g, kl = divmod(kp, R)
        band = np.nonzero(touched[g * R:(g + 1) * R].any(axis=0))[0]
        assert lo[g] == band.min() and band.max() - band.min() < U
        for p in range(K):
            for r in range(s):
                for dk in range(min(U, Hi - lo[g])):
                    v = Gf[p, kp, lo[g] + dk, r * Wo:r * Wo + Mo] / s
                    want[g, :, kl * K + p, 2 * (r * U + dk)] = v.real
                    want[g, :, kl * K + p, 2 * (r * U + dk) + 1] = v.imag
    err = np.abs(T - want).max() / np.abs(Gf).max()
    print(f"MEASURED disco_spectral tables {name} U {U} max err / max|G| {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("planes", [1, 5])
@pytest.mark.parametrize("name", list(SHAPES))
def test_cpu_op_with_numpy_fft_against_the_definition(name, planes):
    ins, outs, ks, grid = SHAPES[name]
    K = D.kernel_size(ks)
    T, lo, U = D.disco_spectral_tables(ins, outs, ks, grid, grid, dtype=np.float64)
    x = torch.randn(planes, 1, *ins, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    m = DiscreteContinuousConvS2(1, 1, ins, outs, ks, grid_in=grid, grid_out=grid, backend="torch")
    ref = m.gather_torch(x)[:, 0]  # [planes, K, Ho, Wo]
    xh = torch.view_as_real(torch.from_numpy(np.fft.rfft(x[:, 0].numpy(), axis=-1)))
    yh = ops.disco_spectral(xh, torch.from_numpy(T)[None], torch.from_numpy(lo), K, U, outs[0], ins[1], outs[1])
    assert yh.shape == (planes, K, outs[0], outs[1] // 2 + 1, 2) and yh.dtype == torch.float64
    y = torch.from_numpy(np.fft.irfft(torch.view_as_complex(yh).numpy(), n=outs[1], axis=-1))
    err = float(((y - ref).flatten(2).norm(dim=2) / ref.flatten(2).norm(dim=2)).max())
    print(f"MEASURED disco_spectral cpu op {name} planes {planes} per-field rel-L2 {err:.2e}")
    assert err < 1e-12


def test_checks_and_info():
    ins, outs, ks, _ = SHAPES["k9"]
    h = D.disco_spectral_table_holder(ins, outs, ks)
    assert h is D.disco_spectral_table_holder(ins, outs, ks) and h is not D.disco_table_holder(ins, outs, ks)
    assert (h.K, h.R, h.s, h.Mo) == (9, 1, 2, 9) and h.table.shape == (2, 9, 9, 16, h.KD)
    assert h.table_bytes == h.table.numel() * 2 and h.lo.dtype == torch.int32
    info = ops.disco_spectral_info(5, *ins, h.K, *outs, h.U, False)
    assert info == f"R=1 KD={h.KD} MT=8 PTL=16 lds={2 * 8 * (16 * (2 * h.KD + 16) + 32)} wgs=18 table_bytes={h.table_bytes}"
    xh = torch.randn(2, ins[0], ins[1] // 2 + 1, 2)
    args = (h.lo, h.K, h.U, outs[0], ins[1], outs[1])
    y = ops.disco_spectral(xh, h.table, *args)
    yb = ops.disco_spectral(xh.bfloat16(), h.table_bf16, *args)
    assert y.dtype == torch.float32 and yb.dtype == torch.bfloat16 and (y - yb.float()).abs().max() < 0.05 * y.abs().max()
    for bad in [(xh, h.table_bf16), (xh.bfloat16(), h.table), (xh, h.table.float())]:  # mixed precisions
        with pytest.raises(RuntimeError, match="must both be"):
            ops.disco_spectral(*bad, *args)
    out = torch.empty_like(y)
    assert ops.disco_spectral_out(xh, h.table, *args, out) is out and torch.equal(out, y)
    assert ops.disco_spectral(xh.to("meta"), h.table, *args).shape == y.shape


@pytest.mark.parametrize("name", ["k9", "s3"])
def test_module_spectral_equals_gather_and_runs_through_onnx(name):
    ins, outs, ks, grid = SHAPES[name]
    torch.manual_seed(5)
    kw = dict(grid_in=grid, grid_out=grid)
    m = DiscreteContinuousConvS2(3, 4, ins, outs, ks, algorithm="spectral", **kw).eval()
    g = DiscreteContinuousConvS2(3, 4, ins, outs, ks, **kw).eval()
    g.load_state_dict(m.state_dict())
    x = torch.randn(2, 3, *ins)
    with torch.no_grad():
        eager, ref = m(x), g.set_backend("torch")(x.double())
    err = float(((eager.double() - ref).flatten(2).norm(dim=2) / ref.flatten(2).norm(dim=2)).max())
    print(f"MEASURED disco_spectral module cpu {name} per-field rel-L2 {err:.2e}")
    assert err < 1e-5  # the table is the bf16 (hi + lo) split of fp32: 2^-17 relative per entry
    data = ex.export(m, (x,))
    nodes = P.load_model(data).graph.node
    assert [n.op_type for n in nodes if n.domain == "com.amd.dft"] == ["r2c", "disco_spectral", "c2r", "fno_pointwise"]
    assert {n.op_type for n in nodes if n.domain != "com.amd.dft"} <= {"Constant", "Reshape"}
    (y,) = OnnxGraph(data, torch.device("cpu")).run(x)
    assert torch.equal(y, eager)
    (ye,) = Engine.build(m, (x,), device="cpu").infer(x)
    assert torch.equal(ye, eager)
    with pytest.raises(ValueError, match="algorithm"):
        DiscreteContinuousConvS2(3, 4, ins, outs, ks, algorithm="auto")
