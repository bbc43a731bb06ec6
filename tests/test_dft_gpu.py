"""GPU correctness of the hand-written Stockham kernels vs an fp64 torch.fft oracle (CPU).

Extends the reference's grid (/root/reference/tests/test_dft.py:124-184: signal_ndim=2,
W=4 only) to every length 1..64, the FourCastNet/FNO lengths (90, 180, 720, 1440), powers of
two, large primes (generic radix), signal_ndim 1/2/3, channel-last dims, bf16 I/O, norms,
pruned (mode-truncated) transforms, input-not-clobbered and hipGraph replay.
"""
import pytest
import torch

import tensorrt_dft_plugins_amd as tdp
from tensorrt_dft_plugins_amd.ops import dft
from helpers import long_fft_tol, rel_l2

pytestmark = pytest.mark.gpu

TOL = 2e-6


def _oracle_rfftn(x, dims, norm="backward"):
    return torch.fft.rfftn(x.double().cpu(), dim=dims, norm=norm)


@pytest.mark.parametrize("n", list(range(1, 65)) + [90, 97, 103, 128, 180, 256, 360, 720, 1000, 1024, 1440, 2048, 4096])
def test_rfft_1d_lengths(device, n):
    torch.manual_seed(n)
    x = torch.randn(5, n, device=device)
    y = tdp.rfft(x)
    ref = torch.fft.rfft(x.double().cpu())
    assert y.shape == ref.shape
    assert rel_l2(y, ref) < TOL * max(1.0, (n.bit_length()))
    # inverse round trip (even lengths are recoverable; odd need n=)
    xr = tdp.irfft(y, n=n)
    assert rel_l2(xr, x) < TOL * max(1.0, n.bit_length())


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 12, 60, 90, 97, 720, 1440])
def test_c2c_1d(device, n):
    torch.manual_seed(0)
    x = torch.randn(3, n, dtype=torch.complex64, device=device)
    y = tdp.fft(x)
    assert rel_l2(y, torch.fft.fft(x.cpu().to(torch.complex128))) < TOL * max(1, n.bit_length())
    z = tdp.ifft(x)
    assert rel_l2(z, torch.fft.ifft(x.cpu().to(torch.complex128))) < TOL * max(1, n.bit_length())


@pytest.mark.parametrize("dft_dim1", [1, 2])
@pytest.mark.parametrize("dft_dim2", [4])
@pytest.mark.parametrize("num_c", [1, 3])
@pytest.mark.parametrize("batch_size", [1, 2])
def test_reference_grid_contrib(device, dft_dim1, dft_dim2, num_c, batch_size):
    """The reference's exact test grid through the contrib Rfft/Irfft ops on the GPU."""
    torch.manual_seed(1)
    x = torch.randn(batch_size, num_c, dft_dim1, dft_dim2)
    y_expected = torch.view_as_real(torch.fft.rfft2(x, dim=(-2, -1), norm="backward"))
    y = tdp.contrib_rfft(x.to(device), signal_ndim=2).cpu()
    assert torch.allclose(y_expected, y, atol=1e-6)
    x_expected = torch.fft.irfft2(torch.view_as_complex(y_expected), dim=(-2, -1), norm="backward")
    x_actual = tdp.contrib_irfft(y_expected.to(device), signal_ndim=2).cpu()
    assert torch.allclose(x_expected, x_actual, atol=1e-6)


@pytest.mark.parametrize("shape,nd", [((2, 720, 1440), 2), ((1, 720, 1440), 2), ((3, 4, 8, 6, 10), 3),
                                      ((2, 90, 180), 2), ((7, 33, 20), 2), ((2, 5, 16, 9, 12), 3),
                                      ((1024,), 1), ((1, 1024), 1)])
@pytest.mark.parametrize("norm", ["backward", "ortho", "forward"])
def test_rfftn_multi(device, shape, nd, norm):
    torch.manual_seed(2)
    x = torch.randn(*shape, device=device)
    dims = list(range(len(shape) - nd, len(shape)))
    y = tdp.rfftn(x, dim=dims, norm=norm)
    ref = _oracle_rfftn(x, dims, norm)
    assert rel_l2(y, ref) < 5e-6
    z = tdp.irfftn(y, s=[shape[d] for d in dims], dim=dims, norm=norm)
    assert rel_l2(z, x) < 5e-6


def test_channel_last_afno_dims(device):
    """FourCastNet AFNO: rfft2 over dims (1, 2) of [B, H, W, C], norm='ortho'."""
    torch.manual_seed(3)
    x = torch.randn(2, 90, 180, 64, device=device)
    y = tdp.rfft2(x, dim=(1, 2), norm="ortho")
    ref = torch.fft.rfft2(x.double().cpu(), dim=(1, 2), norm="ortho")
    assert rel_l2(y, ref) < 5e-6
    z = tdp.irfft2(y, s=(90, 180), dim=(1, 2), norm="ortho")
    assert rel_l2(z, x) < 5e-6
    # odd channel count exercises the unpaired-signal path
    x3 = torch.randn(1, 12, 10, 3, device=device)
    assert rel_l2(tdp.rfft2(x3, dim=(1, 2)), torch.fft.rfft2(x3.double().cpu(), dim=(1, 2))) < 5e-6


def test_bf16_io(device):
    torch.manual_seed(4)
    x = torch.randn(4, 20, 72, 144, device=device).to(torch.bfloat16)
    y = tdp.rfft2(x)  # bf16 in, fp32 out
    ref = torch.fft.rfft2(x.double().cpu())
    assert rel_l2(y, ref) < 5e-6
    yb = tdp.rfft2(x, return_real=True)  # bf16 out
    assert yb.dtype == torch.bfloat16
    assert rel_l2(torch.view_as_complex(yb.float()), ref) < 8e-3
    z = tdp.irfft2(yb, s=(72, 144), out_dtype=torch.bfloat16)
    assert z.dtype == torch.bfloat16
    assert rel_l2(z, x.float()) < 1.5e-2


def test_pruned_modes(device):
    """FNO-style truncation: keep [0,m1) u [H-m1,H) x [0,m2)."""
    torch.manual_seed(5)
    B, C, H, W, m1, m2 = 2, 3, 64, 96, 12, 20
    x = torch.randn(B, C, H, W, device=device)
    y = dft.rfftn_pruned(x, [2, 3], [(m1, m1), (m2, 0)])
    full = torch.fft.rfft2(x.double().cpu())
    ref = torch.cat([full[:, :, :m1, :m2], full[:, :, -m1:, :m2]], dim=2)
    assert y.shape == (B, C, 2 * m1, m2, 2)
    assert rel_l2(torch.view_as_complex(y), ref) < 5e-6
    z = dft.irfftn_pruned(y, [2, 3], [H, W], [(m1, m1), (m2, 0)])
    pad = torch.zeros(B, C, H, W // 2 + 1, dtype=torch.complex128)
    pad[:, :, :m1, :m2] = ref[:, :, :m1]
    pad[:, :, -m1:, :m2] = ref[:, :, m1:]
    zref = torch.fft.irfft2(pad, s=(H, W))
    assert rel_l2(z, zref) < 5e-6


def test_input_not_clobbered(device):
    torch.manual_seed(6)
    y = torch.randn(2, 3, 64, 33, 2, device=device)
    y0 = y.clone()
    tdp.contrib_irfft(y, signal_ndim=2)
    assert torch.equal(y, y0)


def test_irfft_ignores_dc_nyquist_imag(device):
    torch.manual_seed(7)
    X = torch.randn(4, 17, dtype=torch.complex64)
    out = tdp.irfft(X.to(device), n=32).cpu()
    ref = torch.fft.irfft(X.to(torch.complex128), n=32)
    assert rel_l2(out, ref) < 5e-6


def test_deterministic(device):
    x = torch.randn(8, 720, 1440, device=device)
    a = tdp.rfft2(x)
    b = tdp.rfft2(x)
    assert torch.equal(a, b)


def test_hipgraph_capture_replay(device):
    x = torch.randn(2, 720, 1440, device=device)
    y = tdp.contrib_rfft(x, signal_ndim=2)  # warm-up creates the plans
    z = tdp.contrib_irfft(y, signal_ndim=2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yg = tdp.contrib_rfft(x, signal_ndim=2)
        zg = tdp.contrib_irfft(yg, signal_ndim=2)
    x.copy_(torch.randn_like(x))
    g.replay()
    torch.cuda.synchronize()
    assert rel_l2(zg, x) < 5e-6
    assert rel_l2(torch.view_as_complex(yg), torch.fft.rfft2(x.double().cpu())) < 5e-6


def test_native_kernel_is_used(device):
    """The CUDA dispatch key must route to the HIP kernels (no torch.fft fallback)."""
    from torch.profiler import ProfilerActivity, profile

    x = torch.randn(4, 720, 1440, device=device)
    tdp.rfft2(x)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        tdp.rfft2(x)
        torch.cuda.synchronize()
    names = " ".join(e.name for e in prof.events())
    assert "amd_dft" in names and "fft_" in names
    assert "rocfft" not in names.lower()


def test_fixed_kernel_paths(device):
    """The specialised (compile-time) row / column / channel-last kernels against the oracle (the
    generic runtime-radix kernels are covered by the lengths without a fixed configuration, and the
    A/B switch between the two families exists only in tuning builds, csrc/ops/tuning.h)."""
    torch.manual_seed(8)
    for shape in [(3, 720, 1440), (2, 90, 180, 24)]:
        x = torch.randn(*shape, device=device)
        dims = (-2, -1) if len(shape) == 3 else (1, 2)
        y = tdp.rfft2(x, dim=dims)
        assert rel_l2(y, torch.fft.rfft2(x.double().cpu(), dim=dims)) < 5e-6
        z = tdp.irfft2(y, s=[shape[d] for d in dims], dim=dims)
        assert rel_l2(z, x) < 5e-6
        c = torch.randn(*shape, dtype=torch.complex64, device=device)
        assert rel_l2(tdp.fftn(c, dim=dims), torch.fft.fftn(c.cpu().to(torch.complex128), dim=dims)) < 5e-6


def test_finite_check_mode_gpu(device):
    """MI_DFT_CHECK_FINITE=1 turns a NaN output into a Python error (opt-in)."""
    import subprocess
    import sys

    code = ("import torch, tensorrt_dft_plugins_amd as t; t.load_plugins();"
            "x = torch.randn(4, 64, device='cuda'); x[1, 3] = float('nan');"
            "ok = torch.ops.amd_dft.r2c(torch.randn(4, 64, device='cuda'), [1]); torch.cuda.synchronize();\n"
            "try:\n    torch.ops.amd_dft.r2c(x, [1]); print('NOERR')\n"
            "except RuntimeError as e:\n    print('RAISED', 'NaN/Inf' in str(e))\n")
    import os

    env = dict(os.environ, MI_DFT_CHECK_FINITE="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=root)
    assert "RAISED True" in r.stdout, r.stdout + r.stderr[-2000:]


@pytest.mark.parametrize("n", [6553, 8192, 8198, 10007, 20000, 65536, 100003])
def test_long_lengths_four_step_bluestein(device, n):
    """Lengths beyond one LDS-resident pass (limit 6552): four-step composition, and Bluestein
    for primes (10007, 100003) -- cuFFT, the reference's backend, accepts any length."""
    torch.manual_seed(n % 97)
    x = torch.randn(2, n, device=device)
    y = tdp.rfft(x)
    ref = torch.fft.rfft(x.double().cpu())
    tol = long_fft_tol(n)
    assert rel_l2(y, ref) < tol, n
    xr = tdp.irfft(y, n=n)
    assert rel_l2(xr, x) < tol, n
    z = torch.randn(2, n, dtype=torch.complex64, device=device)
    assert rel_l2(tdp.fft(z), torch.fft.fft(z.cpu().to(torch.complex128))) < tol, n
    assert rel_l2(tdp.ifft(z), torch.fft.ifft(z.cpu().to(torch.complex128))) < tol, n


def test_long_length_2d_and_pruned(device):
    torch.manual_seed(3)
    x = torch.randn(2, 12, 9000, device=device)
    y = tdp.rfft2(x)
    assert rel_l2(y, torch.fft.rfft2(x.double().cpu())) < 1e-5
    assert rel_l2(tdp.irfft2(y, s=(12, 9000)), x) < 1e-5
    from tensorrt_dft_plugins_amd.ops import dft as D

    yp = D.rfftn_pruned(x, [1, 2], [(3, 2), (40, 0)])
    full = torch.fft.rfft2(x.double().cpu())
    ref = torch.cat([full[:, :3, :40], full[:, -2:, :40]], 1)
    assert rel_l2(yp, ref) < 1e-5


@pytest.mark.parametrize("shape", [(720, 1440), (1, 720, 1440)])
def test_rfft2_irfft2_720x1440_graph_replays(device, shape):
    """The headline transform (XCD-ordered 4-column tiles) eagerly and under hipGraph replay
    against torch.fft in fp64."""
    torch.manual_seed(11)
    x = torch.randn(*shape)
    ref = torch.view_as_real(torch.fft.rfft2(x.double()))
    xd = x.to(device)
    y = tdp.contrib_rfft(xd, signal_ndim=2)
    assert (y.cpu().double() - ref).norm() / ref.norm() < 2e-6
    z = tdp.contrib_irfft(y, signal_ndim=2)
    assert (z.cpu().double() - x.double()).norm() / x.double().norm() < 2e-6
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tdp.contrib_irfft(tdp.contrib_rfft(xd, signal_ndim=2), signal_ndim=2)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yg = tdp.contrib_rfft(xd, signal_ndim=2)
        zg = tdp.contrib_irfft(yg, signal_ndim=2)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert (yg.cpu().double() - ref).norm() / ref.norm() < 2e-6
    assert (zg.cpu().double() - x.double()).norm() / x.double().norm() < 2e-6
