"""The transposed longitude-Fourier DISCO route on the CPU: the fp64 op with ``torch.fft`` around it against
``disco_t``, the table against the direct DFT of the dense PsiT, the route strings, the module and its export."""
import math

import numpy as np
import pytest
import torch

from tensorrt_dft_plugins_amd import load_plugins
from tensorrt_dft_plugins_amd.models import DiscreteContinuousConvTransposeS2
from tensorrt_dft_plugins_amd.onnx import exporter as ex
from tensorrt_dft_plugins_amd.onnx import proto as P
from tensorrt_dft_plugins_amd.onnx.runner import OnnxGraph
from tensorrt_dft_plugins_amd.ops import disco as D

load_plugins()
ops = torch.ops.amd_dft
EQ, LG = "equiangular", "legendre-gauss"
# name -> (in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, (K, U, KD))
SHAPES = {
    "s2": ((9, 16), (17, 32), (2, 3), EQ, EQ, None, (4, 9, 96)),      # two groups, the last of one row; 17 modes
    "s3": ((6, 12), (12, 36), 2, LG, LG, None, (2, 6, 32)),           # modes 12 .. 18 wrap to nu = 0 .. 6
    "s1": ((12, 20), (12, 20), 3, EQ, LG, None, (3, 12, 96)),         # no conjugated run
    "odd": ((4, 5), (6, 15), 3, EQ, EQ, None, (3, 4, 32)),            # odd nlon: no Nyquist mode
    "k17": ((9, 8), (9, 16), (5, 4), EQ, EQ, None, (17, 9, 320)),     # K > 16; fp32 96 * 3 + 32, bf16 224 + 96
    "kd128": ((16, 8), (16, 8), (2, 3), EQ, EQ, math.pi, (4, 16, 128)),  # fp32 96 + 32, the edge inside a basis plane
    "g3": ((17, 16), (33, 32), 3, EQ, EQ, None, (3, 12, 96)),         # three groups with different lo
}


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_fp64_route_against_disco_t(name, with_bias):
    ins, outs, ks, gi, go, cut, kud = SHAPES[name]
    T, lo, U = D.disco_spectral_transpose_tables(ins, outs, ks, gi, go, cut, dtype=np.float64)
    K = D.kernel_size(ks)
    assert (K, U, T.shape[-1]) == kud and T.shape[:3] == (-(-outs[0] // 16), outs[1] // 2 + 1, 16)
    g = torch.Generator().manual_seed(4)
    z = torch.randn(2, 3, K, *ins, dtype=torch.float64, generator=g)
    bias = torch.randn(3, dtype=torch.float64, generator=g) if with_bias else None
    csr = [torch.from_numpy(a) for a in D.disco_transpose_tables(ins, outs, ks, gi, go, cut, dtype=np.float64)]
    ref = ops.disco_t(z, *csr, *outs, bias)
    zh = torch.view_as_real(torch.fft.rfft(z, dim=-1))
    yh = ops.disco_spectral_t(zh, torch.from_numpy(T)[None], torch.from_numpy(lo), K, U, outs[0], ins[1], outs[1], bias)
    assert yh.shape == (2, 3, outs[0], outs[1] // 2 + 1, 2) and yh.dtype == torch.float64
    y = torch.fft.irfft(torch.view_as_complex(yh), n=outs[1], dim=-1)
    print(f"MEASURED disco_spectral_t fp64 route {name} max err / max|y| {(y - ref).abs().max() / ref.abs().max():.2e}")
    assert (y - ref).abs().max() < 1e-12 * ref.abs().max()


def test_table_against_the_direct_dft_of_dense_psit():
    ins, outs, ks, gi, go, cut, (K, U, _) = SHAPES["s2"]
    (Hi, Wi), (Ho, Wo) = ins, outs
    s = Wo // Wi
    rp, idx, val = D.disco_transpose_tables(ins, outs, ks, gi, go, cut, dtype=np.float64)
    row = np.repeat(np.arange(Ho * s), np.diff(rp))
    psit = np.zeros((K, Hi, Ho, Wo))  # PsiT[p, k', k, D], D = (rho - s d) mod nlon_out
    psit[idx // Wi % K, idx // Wi // K, row // s, (row % s - s * (idx % Wi)) % Wo] = val
    H = psit @ np.exp(-2j * np.pi * np.outer(np.arange(Wo), np.arange(Wo // 2 + 1)) / Wo)  # [p, k', k, mu]
    T, lo, _ = D.disco_spectral_transpose_tables(ins, outs, ks, gi, go, cut, dtype=np.float64)
    want = np.zeros_like(T)
    for k in range(Ho):
        for dk in range(min(U, Hi - lo[k // 16])):
            for p in range(K):
                h = H[p, lo[k // 16] + dk, k]
                want[k // 16, :, k % 16, 2 * (p * U + dk)], want[k // 16, :, k % 16, 2 * (p * U + dk) + 1] = h.real, h.imag
    assert np.abs(T - want).max() <= 1e-13 * np.abs(H).max() and np.abs(psit).sum() == pytest.approx(np.abs(val).sum())


@pytest.mark.parametrize("args,bf,want", [
    ((20, 360, 720, 3, 720, 1440, 16), False, "KD=96 KC=96 chunks=1 MT=8 PTL=16 lds=53760 wgs=8190 table_bytes=199342080"),
    ((64, 180, 360, 9, 180, 360, 24), False, "KD=448 KC=96 chunks=5 MT=8 PTL=16 lds=53760 wgs=1104 table_bytes=62275584"),
    ((64, 180, 360, 9, 180, 360, 24), True,
     "KD=448 KC=224 chunks=2 MT=8 PTL=16 lds=59648 wgs=1104 table_bytes=31137792 bf16=1"),
    ((5, 9, 8, 17, 9, 16, 9), False, "KD=320 KC=96 chunks=4 MT=8 PTL=16 lds=53760 wgs=2 table_bytes=184320"),
    ((5, 9, 8, 17, 9, 16, 9), True, "KD=320 KC=224 chunks=2 MT=8 PTL=16 lds=59648 wgs=2 table_bytes=92160 bf16=1"),
])
def test_info(args, bf, want):
    assert ops.disco_spectral_t_info(*args, bf) == want


def test_holder_dtypes_and_raises():
    ins, outs, ks = SHAPES["k17"][:3]
    h = D.disco_spectral_transpose_table_holder(ins, outs, ks)
    assert h is D.disco_spectral_transpose_table_holder(ins, outs, ks) and h.table.shape == (2, 1, 9, 16, 320)
    assert (h.K, h.U, h.KD, h.s, h.Mo, h.table_bytes) == (17, 9, 320, 2, 9, h.table.numel() * 2)
    zh = torch.randn(2, h.K, ins[0], ins[1] // 2 + 1, 2)
    args = (h.lo, h.K, h.U, outs[0], ins[1], outs[1])
    y, yb = ops.disco_spectral_t(zh, h.table, *args), ops.disco_spectral_t(zh.bfloat16(), h.table_bf16, *args)
    assert y.dtype == torch.float32 and yb.dtype == torch.bfloat16 and (y - yb.float()).abs().max() < 0.05 * y.abs().max()
    for bad in [(zh, h.table_bf16), (zh.bfloat16(), h.table), (zh, h.table.float())]:  # mixed precisions
        with pytest.raises(RuntimeError, match="must both be"):
            ops.disco_spectral_t(*bad, *args)
    out = torch.empty_like(y)
    assert ops.disco_spectral_t_out(zh, h.table, *args, None, out) is out and torch.equal(out, y)
    assert ops.disco_spectral_t(zh.to("meta"), h.table, *args).shape == y.shape
    with pytest.raises(ValueError, match="algorithm"):
        DiscreteContinuousConvTransposeS2(3, 4, ins, outs, ks, algorithm="auto")


def test_module_spectral_on_cpu_and_through_onnx():
    ins, outs, ks, gi, go = (6, 12), (12, 36), 2, LG, LG
    torch.manual_seed(5)
    m = DiscreteContinuousConvTransposeS2(3, 4, ins, outs, ks, grid_in=gi, grid_out=go, algorithm="spectral").eval()
    x = torch.randn(2, 3, *ins)
    with torch.no_grad():
        m.bias.normal_()
        eager, ref = m(x), m.set_backend("torch")(x.double())
    m.set_backend("amd")
    err = float(((eager.double() - ref).flatten(2).norm(dim=2) / ref.flatten(2).norm(dim=2)).max())
    print(f"MEASURED disco_spectral_t module cpu per-field rel-L2 {err:.2e}")
    assert err < 1e-5  # the table is the bf16 (hi + lo) split of fp32: 2^-17 relative per entry
    data = ex.export(m, (x,))
    nodes = P.load_model(data).graph.node
    assert [n.op_type for n in nodes if n.domain == "com.amd.dft"] == ["fno_pointwise", "r2c", "disco_spectral_t", "c2r"]
    assert {n.op_type for n in nodes if n.domain != "com.amd.dft"} <= {"Constant", "Reshape"}
    assert torch.equal(OnnxGraph(data, torch.device("cpu")).run(x)[0], eager)
