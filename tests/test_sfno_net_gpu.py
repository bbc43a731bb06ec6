"""``models.SFNONet`` on the GPU: every line on hand kernels under ``strict_mode`` with no fallback counted, in fp32 and
bf16, eager and as an engine.

Configs: [2, 5, 33, 64] equiangular untruncated and [1, 20, 45, 90] Legendre-Gauss with lmax 23, mmax 13 (the shapes of
tests/test_sht_gpu.py), depth 2, embed 8.  Bounds, per field against the torch backend in fp64: fp32 1e-5 (``TOL`` of
tests/test_sht_gpu.py), bf16 2e-2 (the project's bf16 layer bound; the reference runs on the same bf16 input and
bf16-rounded weights).  Every norm call must be ``instance_norm`` on tensors of the input's dtype.  An unoptimized
engine equals the eager result bit for bit, the optimized one stays within the bounds, and a saved and loaded engine
replays the same bits."""
import pytest
import torch

import test_sfno_net as N
from test_sht_gpu import TOL
from tensorrt_dft_plugins_amd import utils
from tensorrt_dft_plugins_amd.engine import Engine
from tensorrt_dft_plugins_amd.models import SFNOConfig, SFNONet
from tensorrt_dft_plugins_amd.ops import spectral as SP

BF = torch.bfloat16
CONFIGS = [((2, 5, 33, 64), None, None, "equiangular"), ((1, 20, 45, 90), 23, 13, "legendre-gauss")]
IDS = ["2x5x33x64-equiangular", "1x20x45x90-gauss"]


@pytest.fixture()
def strict():
    prev = utils.strict_mode(True)
    SP.fallback_reset()
    try:
        yield
        assert SP.fallback_counts() == {}
    finally:
        utils.strict_mode(prev)


_REFS = {}


def net_and_ref(cfg, bf16):
    """(net on the CPU, x, fp64 torch-backend reference), built once per (config, dtype) and left unchanged."""
    key = (cfg[0], bf16)
    if key not in _REFS:
        shape, lmax, mmax, grid = cfg
        net = N.make_net(seed=11, img_size=shape[2:], in_chans=shape[1], out_chans=3, embed_dim=8, depth=2, lmax=lmax,
                         mmax=mmax, grid=grid)
        x = torch.randn(*shape)
        with torch.no_grad():
            if bf16:
                for p in net.parameters():
                    p.copy_(p.to(BF).float())
                x = x.to(BF)
            ref = net.set_backend("torch")(x.double())
        _REFS[key] = (net.set_backend("amd"), x, ref)
    return _REFS[key]


def spy_norm(monkeypatch):
    calls = []
    real = SP.instance_norm

    def spy(x, weight=None, bias=None, eps=1e-5):
        calls.append((x.dtype, x.is_cuda, float(eps)))
        return real(x, weight, bias, eps)

    monkeypatch.setattr(SP, "instance_norm", spy)
    monkeypatch.setattr(torch.nn.functional, "instance_norm", lambda *a, **k: pytest.fail("a norm left the hand kernel"))
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_sfno_net_gpu(device, strict, cfg, bf16, monkeypatch):
    net, x, ref = net_and_ref(cfg, bf16)
    calls = spy_norm(monkeypatch)
    net = net.to(device)
    try:
        with torch.no_grad():
            out = net(x.to(device))
            again = net(x.to(device))
    finally:
        net.cpu()
    assert out.dtype == x.dtype and out.shape == ref.shape and torch.equal(out, again)
    err = N.field_err(out, ref)
    print(f"MEASURED sfno_net gpu {cfg[0]} {'bf16' if bf16 else 'fp32'} per-field rel-L2 {err:.3e}")
    assert err < (N.TOL_BF16 if bf16 else TOL)
    assert len(calls) == 2 * 2 * 2 and all(c == (x.dtype, True, 1e-6) for c in calls)


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_sfno_net_engine_gpu(device, strict, cfg, bf16, tmp_path):
    net, x, ref = net_and_ref(cfg, bf16)
    tol = N.TOL_BF16 if bf16 else TOL
    xd = x.to(device)
    net = net.to(device)
    try:
        with torch.no_grad():
            eager = net(xd).clone()
    finally:
        net.cpu()
    plain = Engine.build(net, (x,), device=device, optimize=False)
    assert plain.use_graph
    (y,) = plain.infer(xd)
    assert y.dtype == x.dtype and torch.equal(y, eager)
    (y2,) = plain.infer(xd)
    assert torch.equal(y2, eager)
    opt = Engine.build(net, (x,), device=device)
    (yo,) = opt.infer(xd)
    err = N.field_err(yo, ref)
    print(f"MEASURED sfno_net engine (optimized) {cfg[0]} {'bf16' if bf16 else 'fp32'} per-field rel-L2 {err:.3e}")
    assert err < tol
    p = str(tmp_path / "sfno.engine")
    plain.save(p)
    (yl,) = Engine.load(p, device=device).infer(xd)
    assert torch.equal(yl, eager)


@pytest.mark.gpu
def test_stock_instance_norm_runs_the_hand_kernel_gpu(device, strict):
    """A stock-exported ``nn.InstanceNorm2d`` in an unoptimized engine is ``instance_norm`` on the device."""
    torch.manual_seed(2)
    m = torch.nn.InstanceNorm2d(5, eps=1e-6, affine=True).eval()
    with torch.no_grad():
        m.weight.normal_()
        m.bias.normal_()
    x = torch.randn(2, 5, 33, 64)
    eng = Engine.build(m, (x,), device=device, optimize=False)
    (y,) = eng.infer(x.to(device))
    assert torch.equal(y, SP.instance_norm(x.to(device), m.weight.to(device), m.bias.to(device), 1e-6))
    ref = torch.nn.functional.instance_norm(x.double(), weight=m.weight.double(), bias=m.bias.double(), eps=1e-6)
    assert N.field_err(y, ref.detach()) < TOL
