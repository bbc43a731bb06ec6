"""The fused FNO layer tail above 32 channels: the route (``fno_c2r_pw_info``), the wide tail kernel
(csrc/spectral/fno_c2r_pw_wide.hip) against the op's CPU implementation (fp64 irfft, x upcast to fp32), the kernel the
ops really launch, and FNO2d at width 64.

Tolerances are the project's: fp32 I/O runs the bf16x3 split on both GEMM halves (2e-5), bf16 I/O has bf16 operands
and a bf16 store (1e-2; 8e-3 for the spectral-only tail, tests/test_fno.py).  Errors are taken per output channel
(the maximum over channels of that channel's rel-L2), so one wrong 16-channel tile cannot be averaged away.  The
spectrum is scaled so that the spectral term and the convolution term are both O(1): an error in either shows."""
import re

import pytest
import torch

from tensorrt_dft_plugins_amd.models import FNO2d, FNOConfig
from helpers import rel_l2


def _fields(info):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", info)}


# ------------------------------------------------------------------------------------------ CPU tier
# the shapes of tests/test_fno.py::test_fno_c2r_pw_kernel_gpu: (Cin, Cout, W, m)
NARROW = [(20, 20, 1440, 32), (7, 13, 200, 20), (32, 32, 720, 64), (4, 16, 64, 5)]
WIDE = [(33, 16), (16, 33), (64, 64), (128, 128), (7, 40), (300, 65), (0, 33), (0, 128)]


@pytest.mark.parametrize("bf16", [False, True])
def test_fno_c2r_pw_info_routes(bf16):
    info = torch.ops.amd_dft.fno_c2r_pw_info
    for cin, cout, W, m in NARROW:
        s = info(cin, cout, m, W, bf16)
        assert s.startswith("fused "), s
        f = _fields(s)
        assert f["ks"] == -(-m // 16) and f["co"] == (1 if cout <= 16 else 2) and f["chunk"] == (128 if bf16 else 64), s
    assert info(0, 20, 32, 1440, bf16).startswith("fused ")  # fno_c2r at a narrow width
    for cin, cout in WIDE:
        for W, m in ((1440, 32), (64, 5), (200, 20)):
            s = info(cin, cout, m, W, bf16)
            assert s.startswith("wide "), (cin, cout, W, m, s)
            f = _fields(s)
            assert f["slabs"] == -(-cin // 32) and f["otiles"] == -(-cout // 16), s
            assert f["groups"] == -(-f["otiles"] // 4) and f["x3"] == (0 if bf16 else 1), s
            assert f["ks"] == -(-m // 16) and f["chunk"] == 64, s
    for cin in (64, 0):
        assert info(cin, 64, 65, 1440, bf16) == "split"    # m > 64
        assert info(cin, 64, 20, 100, bf16) == "split"     # W % 8 != 0
        assert info(cin, 64, 64, 8200, bf16) == "split"    # 129 chunks x 64 rotations > the 2048 LDS entries
        assert info(cin, 64, 64, 2048, bf16).startswith("wide ")  # 32 x 64 = 2048: the last W that fits at m = 64
    for bad in ((64, 0, 8, 64), (64, 64, 0, 64), (64, 64, 8, 0), (64, -1, 8, 64), (-1, 64, 8, 64)):
        with pytest.raises(RuntimeError):
            info(*bad, bf16)


def test_fno_c2r_pw_info_reports_where_the_weights_live():
    """``wl``: the wide kernel stages the 1x1 weights in LDS (its WL instances) while they fit beside the tables."""
    info = torch.ops.amd_dft.fno_c2r_pw_info
    for bf16 in (False, True):
        assert _fields(info(64, 64, 16, 128, bf16))["wl"] == 1
        assert _fields(info(300, 65, 5, 72, bf16))["wl"] == (1 if bf16 else 0)  # one plane of fragments fits
        assert _fields(info(521, 65, 8, 64, bf16))["wl"] == 0
        assert _fields(info(0, 65, 5, 72, bf16))["wl"] == 0  # fno_c2r has no weights


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fno_c2r_pw_cpu_out_variant(dt):
    """A NaN-filled ``out`` equals the allocating op's result bit for bit; a wrong-shape, wrong-dtype or
    non-contiguous ``out`` is an error, never a copy."""
    op, op_out = torch.ops.amd_dft.fno_c2r_pw, torch.ops.amd_dft.fno_c2r_pw_out
    g = torch.Generator().manual_seed(44)
    yw = torch.randn(2, 9, 3, 5, 2, generator=g)
    x = torch.randn(2, 12, 3, 16, generator=g).to(dt)
    wc, b = torch.randn(9, 12, generator=g), torch.randn(9, generator=g)
    for bias, gelu in ((b, True), (None, False)):
        ref = op(yw, x, wc, bias, gelu)
        out = torch.full(ref.shape, float("nan"), dtype=dt)
        assert op_out(yw, x, wc, bias, gelu, out) is out
        assert torch.equal(out, ref)
    with pytest.raises(RuntimeError, match="out must be"):
        op_out(yw, x, wc, b, True, torch.empty(2, 12, 3, 16, dtype=dt))
    with pytest.raises(RuntimeError, match="out must be"):
        op_out(yw, x, wc, b, True, torch.empty(2, 9, 3, 32, dtype=dt)[..., ::2])
    with pytest.raises(RuntimeError, match="out must be"):
        op_out(yw, x, wc, b, True, torch.empty(2, 9, 3, 16, dtype=torch.float64))
    m = op_out(yw.to("meta"), x.to("meta"), wc.to("meta"), None, True, torch.empty(2, 9, 3, 16, dtype=dt, device="meta"))
    assert m.device.type == "meta" and m.shape == (2, 9, 3, 16) and m.dtype == dt


# ------------------------------------------------------------------------------------------ GPU tier
def _chan_err(out, ref):
    """max over output channels of the channel's rel-L2 against the reference."""
    o = out.detach().cpu().double().transpose(0, 1).reshape(ref.shape[1], -1)
    r = ref.double().transpose(0, 1).reshape(ref.shape[1], -1)
    num, den = (o - r).norm(dim=1), r.norm(dim=1)
    return float(torch.where(den > 0, num / den, num).max())


# (B, Cin, Cout, H, W, m, gelu, bias): one full group; last slab and last group ragged, chunks 64 * 3 + 8, units
# crossing row and batch boundaries; odd m with Cin <= 32; Cout <= 32 with m just above 32; m at the limit, two
# groups, four slabs (fp32: weights from global memory); W below one tile; weights beyond LDS in both dtypes, with
# 16-byte (300) and per-element (521) weight loads
CASES = [(1, 64, 64, 2, 128, 16, True, True), (2, 33, 65, 3, 200, 20, True, True), (1, 7, 40, 2, 72, 5, False, False),
         (1, 96, 16, 2, 64, 33, True, True), (1, 128, 128, 1, 1440, 64, True, True), (3, 40, 48, 5, 8, 4, True, False),
         (1, 300, 65, 2, 72, 5, True, True), (1, 521, 65, 1, 64, 8, True, True)]
TOL = {torch.float32: 2e-5, torch.bfloat16: 1e-2}
TOL_C2R = {torch.float32: 2e-5, torch.bfloat16: 8e-3}
_cache = {}


def _inputs(case, dt):
    """inputs and the CPU op's result for a case, computed once and shared (never modified)."""
    key = (case, dt)
    if key not in _cache:
        B, Ci, Co, H, W, m, gelu, bias = case
        g = torch.Generator().manual_seed(41)
        yw = torch.randn(B, Co, H, m, 2, generator=g) / (2 * m) ** 0.5
        x = torch.randn(B, Ci, H, W, generator=g).to(dt)
        wc = torch.randn(Co, Ci, generator=g) / Ci ** 0.5
        b = torch.randn(Co, generator=g) if bias else None
        ref = torch.ops.amd_dft.fno_c2r_pw(yw, x.float(), wc, b, gelu)
        _cache[key] = (yw, x, wc, b, ref)
    return _cache[key]


def _dev(device, *ts):
    return tuple(None if t is None else t.to(device) for t in ts)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_wide_tail_kernel_gpu(device, case, dt):
    B, Ci, Co, H, W, m, gelu, bias = case
    assert torch.ops.amd_dft.fno_c2r_pw_info(Ci, Co, m, W, dt == torch.bfloat16).startswith("wide ")
    yw, x, wc, b, ref = _inputs(case, dt)
    out = torch.ops.amd_dft.fno_c2r_pw(*_dev(device, yw, x, wc, b), gelu)
    assert out.dtype == dt and out.shape == ref.shape
    err = _chan_err(out, ref)
    print(f"wide tail {case} {dt}: {err:.3e}")
    assert err < TOL[dt], (case, dt, err)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 40, 3, 200, 20), (1, 65, 2, 72, 5), (3, 40, 5, 8, 4)],
                         ids=lambda s: "x".join(map(str, s)))
def test_wide_c2r_kernel_gpu(device, shape, dt):
    """fno_c2r above 32 output channels: the spectral-only form of the wide kernel."""
    B, Co, H, W, m = shape
    assert torch.ops.amd_dft.fno_c2r_pw_info(0, Co, m, W, dt == torch.bfloat16).startswith("wide ")
    yw = torch.randn(B, Co, H, m, 2, generator=torch.Generator().manual_seed(42)) / (2 * m) ** 0.5
    ref = torch.ops.amd_dft.fno_c2r(yw, W)
    out = torch.ops.amd_dft.fno_c2r(yw.to(device), W, dt)
    assert out.dtype == dt and out.shape == (B, Co, H, W)
    err = _chan_err(out, ref)
    print(f"wide c2r {shape} {dt}: {err:.3e}")
    assert err < TOL_C2R[dt], (shape, dt, err)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_wide_tail_views_gpu(device, dt):
    """yw as a view at an odd float2 offset (off the 16-byte loads' boundary) and x as a non-contiguous view give
    exactly what their contiguous copies give."""
    case = CASES[1]
    B, Ci, Co, H, W, m, gelu, _ = case
    yw, x, wc, b, ref = _inputs(case, dt)
    ywd, xd, wd, bd = _dev(device, yw, x, wc, b)
    want = torch.ops.amd_dft.fno_c2r_pw(ywd, xd, wd, bd, gelu)
    flat = torch.empty(yw.numel() + 2, device=device)
    ywv = flat[2:].view(yw.shape).copy_(ywd)
    assert ywv.data_ptr() % 16 == 8
    xv = torch.empty(B, Ci, H, 2 * W, dtype=dt, device=device)[..., ::2].copy_(xd)
    assert not xv.is_contiguous()
    out = torch.ops.amd_dft.fno_c2r_pw(ywv, xv, wd, bd, gelu)
    assert torch.equal(out, want)
    assert _chan_err(out, ref) < TOL[dt]
    assert torch.equal(torch.ops.amd_dft.fno_c2r(ywv, W, dt), torch.ops.amd_dft.fno_c2r(ywd, W, dt))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_wide_tail_deterministic_gpu(device, dt):
    case = CASES[1]
    yw, x, wc, b, _ = _inputs(case, dt)
    args = _dev(device, yw, x, wc, b) + (case[6],)
    assert torch.equal(torch.ops.amd_dft.fno_c2r_pw(*args), torch.ops.amd_dft.fno_c2r_pw(*args))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_wide_tail_route_is_taken_gpu(device, dt):
    """One 64 -> 64 tail launches the wide kernel and neither the pointwise nor an FFT kernel."""
    from torch.profiler import ProfilerActivity, profile

    yw, x, wc, b, _ = _inputs(CASES[0], dt)
    args = _dev(device, yw, x, wc, b) + (True,)
    torch.ops.amd_dft.fno_c2r_pw(*args)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        torch.ops.amd_dft.fno_c2r_pw(*args)
        torch.cuda.synchronize()
    names = " ".join(e.name for e in prof.events())
    assert "fno_c2r_pw_wide_kernel" in names, names
    assert "fno_pointwise" not in names and "fft_" not in names, names


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fno2d_width64_strict_gpu(device, dt):
    """FNO2d at width 64 (in_chans=3, two layers) under strict mode: every op on its hand kernel, the layer tails on
    the wide fused kernel.  Bounds as tests/test_fno_channels.py::test_fno2d_any_channels_strict_gpu."""
    from tensorrt_dft_plugins_amd import utils
    from tensorrt_dft_plugins_amd.ops import spectral as S

    torch.manual_seed(43)
    cfg = FNOConfig(img_size=(48, 64), in_chans=3, out_chans=1, width=64, modes1=4, modes2=5, n_layers=2,
                    proj_hidden=48)
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
    print(f"FNO2d in=3 width=64 {dt}: rel-L2 {err:.3e}")
    assert err < (1e-4 if dt == torch.float32 else 2e-2)
