"""FNO 1x1 convolutions at any channel count: the pointwise kernel routing (``fno_pointwise_info``), the MFMA
pointwise kernel (csrc/spectral/fno_pointwise_mfma.hip) against an fp64 conv2d reference, and FNO2d / the contrib
engine at channel counts outside the seven register-resident ``fno_pointwise`` instances (Darcy's ``in_chans=3``,
widths above the fused tail's 32).

Tolerances are the project's: fp32 I/O runs the bf16x3 split (2e-5, tests/test_gemm_ragged.py), bf16 I/O has bf16
operands and a bf16 store (1e-2, tests/test_fno.py); the kernel errors are taken per output channel (the maximum over
channels of that channel's rel-L2), so one wrong 16-channel tile cannot be averaged away."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tensorrt_dft_plugins_amd.models import FNO2d, FNOConfig
from helpers import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXED = (4, 8, 16, 20, 32, 64, 128)


def _fields(info):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", info)}


# ------------------------------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("bf16", [False, True])
def test_fno_pointwise_info_routes(bf16):
    info = torch.ops.amd_dft.fno_pointwise_info
    for cin in FIXED:
        s = info(cin, 20, bf16, 720 * 1440)
        assert s.startswith("fixed ") and _fields(s)["cin"] == cin, s
        assert _fields(s)["vp"] == (4 if cin <= 32 else 1), s
        assert _fields(info(cin, 20, bf16, 63))["vp"] == 1
    for cin in (1, 3, 12, 24, 31, 33, 40, 48, 96, 256):
        for cout in (1, 16, 17, 65):
            s = info(cin, cout, bf16, 720 * 1440)
            assert s.startswith("mfma "), s
            f = _fields(s)
            assert f["slabs"] == -(-cin // 32) and f["otiles"] == -(-cout // 16), s
            assert f["groups"] == -(-f["otiles"] // 4) and f["x3"] == (0 if bf16 else 1) and f["vp"] == 4, s
        assert _fields(info(cin, 8, bf16, 4 * 7 + 1))["vp"] == 1  # P % 4 != 0: per-element I/O
    with pytest.raises(RuntimeError):
        info(0, 4, bf16, 16)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fno_pointwise_cpu_out_variant(dt):
    """A NaN-filled ``out`` equals the allocating op's result bit for bit; a wrong-shape, wrong-dtype or
    non-contiguous ``out`` is an error, never a copy."""
    op, op_out = torch.ops.amd_dft.fno_pointwise, torch.ops.amd_dft.fno_pointwise_out
    g = torch.Generator().manual_seed(36)
    x, s = torch.randn(2, 12, 5, 7, generator=g).to(dt), torch.randn(2, 9, 5, 7, generator=g).to(dt)
    w, b = torch.randn(9, 12, generator=g), torch.randn(9, generator=g)
    for spec, bias, gelu in ((s, b, True), (None, None, False)):
        ref = op(spec, x, w, bias, gelu)
        out = torch.full(ref.shape, float("nan"), dtype=dt)
        assert op_out(spec, x, w, bias, gelu, out) is out
        assert torch.equal(out, ref)
    with pytest.raises(RuntimeError, match="out must be"):
        op_out(s, x, w, b, True, torch.empty(2, 12, 5, 7, dtype=dt))
    with pytest.raises(RuntimeError, match="out must be"):
        op_out(s, x, w, b, True, torch.empty(2, 9, 5, 14, dtype=dt)[..., ::2])
    with pytest.raises(RuntimeError, match="out must be"):
        op_out(s, x, w, b, True, torch.empty(2, 9, 5, 7, dtype=torch.float64))
    m = op_out(None, x.to("meta"), w.to("meta"), None, True, torch.empty(2, 9, 5, 7, dtype=dt, device="meta"))
    assert m.device.type == "meta" and m.shape == (2, 9, 5, 7) and m.dtype == dt


def _any_channel_cfg(img, width=40):
    return FNOConfig(img_size=img, in_chans=3, out_chans=1, width=width, modes1=4, modes2=5, n_layers=2,
                     proj_hidden=48)


def test_fno2d_any_channels_amd_cpu():
    torch.manual_seed(30)
    cfg = _any_channel_cfg((24, 32))
    m = FNO2d(cfg, backend="torch").eval()
    x = torch.randn(2, 3, 24, 32)
    with torch.no_grad():
        ref = m(x)
        out = m.set_backend("amd")(x)
    assert out.shape == (2, 1, 24, 32)
    assert rel_l2(out, ref) < 1e-5


def test_standalone_amd_block_fresh_process():
    """A standalone amd FNOBlock (and SpectralConv2d) loads the op library itself: no prior load_plugins()."""
    code = ("import torch\n"
            "from tensorrt_dft_plugins_amd.models.fno import FNOBlock\n"
            "torch.manual_seed(0)\n"
            "blk = FNOBlock(24, 3, 4, backend='amd')\n"
            "x = torch.randn(1, 24, 12, 16)\n"
            "with torch.no_grad():\n"
            "    y = blk(x)\n"
            "    s = blk.spectral(x)\n"
            "    blk.backend = blk.spectral.backend = 'torch'\n"
            "    r = blk(x)\n"
            "assert y.shape == (1, 24, 12, 16) and s.shape == y.shape\n"
            "assert float((y - r).norm() / r.norm()) < 1e-5\n"
            "print('block ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and "block ok" in r.stdout, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------ GPU tier
def _chan_err(out, ref):
    """max over output channels of the channel's rel-L2 against the fp64 reference."""
    o = out.detach().cpu().double().transpose(0, 1).reshape(ref.shape[1], -1)
    r = ref.transpose(0, 1).reshape(ref.shape[1], -1)
    num, den = (o - r).norm(dim=1), r.norm(dim=1)
    return float(torch.where(den > 0, num / den, num).max())


def _reference(x, w, s, b, gelu):
    y = F.conv2d(x.double(), w.double()[:, :, None, None], None if b is None else b.double())
    if s is not None:
        y = y + s.double()
    return F.gelu(y) if gelu else y


# (B, Cin, Cout, H, W): single value; ragged everything; two K slabs with one live row in the second and two output
# tiles with one live column in the second (33 -> 17); more than one output group (65); 8 slabs; P around the 64-pixel
# wave tile (odd P and bf16 rows off the 8-byte boundary take the per-element path)
CASES = [(1, 1, 1, 1, 1), (3, 3, 5, 7, 9), (2, 12, 40, 5, 13), (1, 31, 16, 8, 8), (1, 33, 17, 9, 7),
         (2, 40, 40, 16, 24), (1, 96, 65, 3, 21), (1, 256, 48, 4, 16), (1, 24, 24, 1, 63), (1, 24, 24, 1, 64),
         (1, 24, 24, 1, 65)]
TOL = {torch.float32: 2e-5, torch.bfloat16: 1e-2}


def _inputs(case, dt, seed):
    B, Ci, Co, H, W = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci, H, W, generator=g).to(dt)
    s = torch.randn(B, Co, H, W, generator=g).to(dt)
    w = torch.randn(Co, Ci, generator=g) / Ci ** 0.5
    b = torch.randn(Co, generator=g)
    return x, s, w, b


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_pointwise_mfma_kernel_gpu(device, case, dt):
    assert torch.ops.amd_dft.fno_pointwise_info(case[1], case[2], dt == torch.bfloat16, case[3] * case[4]).startswith("mfma")
    x, s, w, b = _inputs(case, dt, 31)
    xd, sd, wd, bd = (t.to(device) for t in (x, s, w, b))
    for use_spec in (True, False):
        for use_bias in (True, False):
            for gelu in (True, False):
                ref = _reference(x, w, s if use_spec else None, b if use_bias else None, gelu)
                args = (sd if use_spec else None, xd, wd, bd if use_bias else None, gelu)
                out = torch.ops.amd_dft.fno_pointwise(*args)
                assert out.dtype == dt and out.shape == ref.shape
                err = _chan_err(out, ref)
                print(f"pointwise mfma {case} {dt} spec={use_spec} bias={use_bias} gelu={gelu}: {err:.3e}")
                assert err < TOL[dt], (case, dt, use_spec, use_bias, gelu, err)
                assert torch.equal(out, torch.ops.amd_dft.fno_pointwise(*args))  # no atomics: bit-reproducible


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_pointwise_mfma_storage_offset_views_gpu(device, dt):
    """x and spec as views one element into their storage: rows off the vector boundary, per-element I/O."""
    case = (2, 40, 40, 16, 24)
    B, Ci, Co, H, W = case
    x, s, w, b = _inputs(case, dt, 32)
    xv = torch.empty(x.numel() + 1, dtype=dt, device=device)[1:].view(x.shape).copy_(x)
    sv = torch.empty(s.numel() + 1, dtype=dt, device=device)[1:].view(s.shape).copy_(s)
    assert xv.storage_offset() == 1 and sv.storage_offset() == 1 and xv.is_contiguous()
    ref = _reference(x, w, s, b, True)
    out = torch.ops.amd_dft.fno_pointwise(sv, xv, w.to(device), b.to(device), True)
    assert out.dtype == dt
    assert _chan_err(out, ref) < TOL[dt]
    assert torch.equal(out, torch.ops.amd_dft.fno_pointwise(sv, xv, w.to(device), b.to(device), True))
    # the same values through the aligned (vector I/O) path: same products in the same order
    assert torch.equal(out, torch.ops.amd_dft.fno_pointwise(s.to(device), x.to(device), w.to(device), b.to(device), True))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [2, 12])
def test_fno_mix_wide_channels_gpu(device, B):
    """Mode mixing at channel counts whose operand tiles exceed the MFMA kernel's LDS (width 40): the split-K stream
    kernel in batch chunks of 8, no ATen fallback; fp32 FMAs against the fp64 einsum (tests/test_fno.py's 1e-5)."""
    from tensorrt_dft_plugins_amd.ops import spectral as S

    torch.manual_seed(35)
    xm = torch.randn(B, 40, 37, 2)
    w = torch.randn(40, 33, 37, 2)
    ref = torch.einsum("bim,iom->bom", torch.view_as_complex(xm.double()), torch.view_as_complex(w.double()))
    S.fallback_reset()
    out = torch.ops.amd_dft.fno_mix(xm.to(device), w.to(device))
    assert S.fallback_counts() == {}
    assert rel_l2(torch.view_as_complex(out.cpu().contiguous()), ref) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("width", [24, 40])
def test_fno2d_any_channels_strict_gpu(device, width, dt):
    """in_chans=3 (MFMA lift), width 24 (fused tail + MFMA projection) / 40 (tail through c2r + MFMA pointwise),
    proj_hidden=48 (MFMA), under strict mode: every op on its hand kernel.  Bounds: test_fno2d_gpu's 1e-4 for fp32;
    bf16 activations against the fp32 torch model 2e-2, the project's bf16 FNO bound (tests/test_fno.py) -- five
    layers, each rounding its weights and its output to bf16 (2^-9 max, ~1.1e-3 rms each)."""
    from tensorrt_dft_plugins_amd import utils
    from tensorrt_dft_plugins_amd.ops import spectral as S

    torch.manual_seed(33)
    cfg = _any_channel_cfg((48, 64), width)
    m = FNO2d(cfg, backend="torch").to(device).eval()
    x = torch.randn(2, 3, 48, 64, device=device)
    prev = utils.strict_mode(True)
    try:
        with torch.no_grad():
            ref = m(x)
            S.fallback_reset()
            out = m.set_backend("amd")(x.to(dt))
        assert S.fallback_counts() == {}
    finally:
        utils.strict_mode(prev)
    assert out.dtype == dt and out.shape == (2, 1, 48, 64)
    err = rel_l2(out.float(), ref)
    print(f"FNO2d in=3 width={width} {dt}: rel-L2 {err:.3e}")
    assert err < (1e-4 if dt == torch.float32 else 2e-2)


@pytest.mark.gpu
def test_contrib_engine_any_channels_gpu(device):
    """The contrib export of the width-40, in_chans=3 model: the lift and both projections are rewritten to
    fno_pointwise (verified on the device), nothing is rejected, and the engine matches the torch model."""
    from tensorrt_dft_plugins_amd.engine import Engine
    from tensorrt_dft_plugins_amd.onnx import exporter as ex
    from tensorrt_dft_plugins_amd.onnx.optimizer import _precision_tol

    torch.manual_seed(34)
    cfg = _any_channel_cfg((48, 64))
    m = FNO2d(cfg, backend="contrib").eval()
    ref = FNO2d(cfg, backend="torch").eval()
    ref.load_state_dict(m.state_dict())
    x = torch.randn(2, 3, 48, 64)
    with torch.no_grad():
        want = ref(x)
    eng = Engine.build(ex.export(m, x), shapes=[list(x.shape)], device="cuda")
    rep = eng.optimize_report
    assert not [r for r in rep.rejected if r["pattern"].startswith("pointwise_conv")], rep.rejected
    assert not rep.rejected, rep.rejected
    assert rep.count("pointwise_conv") == 2 and rep.count("pointwise_conv_gelu") == 1, rep.applied
    (y,) = eng.infer(x.to(device))
    err = rel_l2(y, want)
    print(f"contrib FNO2d engine in=3 width=40: rel-L2 {err:.3e}")
    assert err < _precision_tol(torch.float32)
