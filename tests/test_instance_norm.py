"""``instance_norm`` on CPU tensors (the ops' ATen kernels), its Meta kernels, error checks, ``instance_norm_info``,
export and the runner's stock ``InstanceNormalization`` operator.  The gfx950 kernels: tests/test_instance_norm_gpu.py."""
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tensorrt_dft_plugins_amd import load_plugins
from tensorrt_dft_plugins_amd.onnx import exporter as ex
from tensorrt_dft_plugins_amd.onnx import proto as P
from tensorrt_dft_plugins_amd.onnx.runner import OnnxGraph
from tensorrt_dft_plugins_amd.ops import spectral as SP

load_plugins()
BF = torch.bfloat16
ops = torch.ops.amd_dft


def _ref(x, w, b, eps):
    return F.instance_norm(x.double(), weight=None if w is None else w.double(), bias=None if b is None else b.double(),
                           eps=eps)


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (1, 2, 33, 64), (2, 4, 50), (1, 2, 3, 4, 5)], ids=str)
@pytest.mark.parametrize("kind", ["normal", "ill"])
def test_instance_norm_cpu_against_fp64(shape, kind):
    torch.manual_seed(3)
    x = torch.randn(*shape)
    if kind == "ill":
        x = 1000.0 + 0.1 * x
    w, b = torch.randn(shape[1]), torch.randn(shape[1])
    for eps in (1e-5, 1e-6):
        ref = _ref(x, w, b, eps)
        out = SP.instance_norm(x, w, b, eps)
        assert out.shape == x.shape and out.dtype == torch.float32
        # the CPU kernel is fp64 math rounded once
        assert torch.all((out.double() - ref).abs() <= 2.0 ** -23 * ref.abs().max())
        st = ops.instance_norm_stats(x, eps)
        flat = x.double().reshape(shape[0], shape[1], -1)
        assert st.shape == (shape[0], shape[1], 2) and st.dtype == torch.float32
        assert torch.equal(st[..., 0], flat.mean(-1).float())
        assert torch.allclose(st[..., 1].double(), (flat.var(-1, unbiased=False) + eps).rsqrt(), rtol=1e-6)
    xb = x.to(BF)
    ob = SP.instance_norm(xb, w.to(BF), b, 1e-5)
    assert ob.dtype == BF
    refb = _ref(xb, w.to(BF), b, 1e-5)
    assert torch.all((ob.double() - refb).abs() <= 2.0 ** -8 * refb.abs() + 1e-30)


@pytest.mark.parametrize("absent", ["weight", "bias", "both"])
def test_instance_norm_absent_affine(absent):
    torch.manual_seed(4)
    x, w, b = torch.randn(2, 3, 5, 6), torch.randn(3), torch.randn(3)
    w = None if absent in ("weight", "both") else w
    b = None if absent in ("bias", "both") else b
    assert torch.allclose(SP.instance_norm(x, w, b).double(), _ref(x, w, b, 1e-5), atol=1e-6)
    out = torch.empty_like(x)
    assert ops.instance_norm_out(x, w, b, 1e-5, out) is out
    assert torch.equal(out, SP.instance_norm(x, w, b))


def test_instance_norm_meta_shapes():
    for dt in (torch.float32, BF):
        x = torch.empty(2, 3, 7, 9, dtype=dt, device="meta")
        w = torch.empty(3, device="meta")
        y = ops.instance_norm(x, w, None, 1e-5)
        assert y.shape == x.shape and y.dtype == dt and y.device.type == "meta"
        st = ops.instance_norm_stats(x, 1e-5)
        assert st.shape == (2, 3, 2) and st.dtype == torch.float32


def test_instance_norm_errors():
    x, w, b = torch.randn(2, 3, 4, 5), torch.randn(3), torch.randn(3)
    for bad in (x.double(), x.half(), x.to(torch.int32)):
        with pytest.raises(RuntimeError, match="float32 or bfloat16"):
            ops.instance_norm(bad, None, None, 1e-5)
        with pytest.raises(RuntimeError, match="float32 or bfloat16"):
            ops.instance_norm_stats(bad, 1e-5)
    with pytest.raises(RuntimeError, match="more than 1 spatial element"):
        ops.instance_norm(torch.randn(2, 3, 1, 1), None, None, 1e-5)
    with pytest.raises(RuntimeError, match="more than 1 spatial element"):
        ops.instance_norm_stats(torch.randn(2, 3, 1), 1e-5)
    with pytest.raises(RuntimeError, match="spatial"):
        ops.instance_norm(torch.randn(2, 3), None, None, 1e-5)
    with pytest.raises(RuntimeError, match="weight must be"):
        ops.instance_norm(x, torch.randn(4), b, 1e-5)
    with pytest.raises(RuntimeError, match="bias must be"):
        ops.instance_norm(x, w, torch.randn(3, 1), 1e-5)
    with pytest.raises(RuntimeError, match="weight must be float32"):
        ops.instance_norm(x, w.double(), b, 1e-5)
    with pytest.raises(RuntimeError, match="bias must be float32"):
        ops.instance_norm(x, w, b.to(BF), 1e-5)  # bf16 per-channel arguments go with a bf16 x only
    with pytest.raises(RuntimeError, match="out must be"):
        ops.instance_norm_out(x, w, b, 1e-5, torch.empty(2, 3, 4, 6))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.instance_norm_out(x, w, b, 1e-5, torch.empty(2, 3, 4, 5, dtype=BF))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.instance_norm_out(x, w, b, 1e-5, torch.empty(2, 3, 5, 4).transpose(-1, -2))


def test_instance_norm_info_routes():
    fields = {"route", "S", "chunk", "vec", "lds", "wgs"}
    for bf16 in (False, True):
        s = ops.instance_norm_info(64, 45 * 90, bf16)
        f = dict(re.findall(r"(\w+)=(\w+)", s))
        assert set(f) == fields and f["route"] == "resident" and f["S"] == "1" and f["chunk"] == str(45 * 90)
        assert f["wgs"] == "64" and f["vec"] == ("8" if bf16 else "4") and int(f["lds"]) >= 45 * 90 * 4
        s = ops.instance_norm_info(20, 720 * 1440, bf16)
        f = dict(re.findall(r"(\w+)=(\w+)", s))
        assert set(f) == fields and f["route"] == "split"
        S, chunk = int(f["S"]), int(f["chunk"])
        assert S >= 2 and (S - 1) * chunk < 720 * 1440 <= S * chunk and int(f["wgs"]) == 20 * S >= 256
        assert chunk * 4 <= int(f["lds"]) <= 160 * 1024
    # few large planes are cut finer than many
    one = int(re.search(r"S=(\d+)", ops.instance_norm_info(1, 1 << 20, False)).group(1))
    many = int(re.search(r"S=(\d+)", ops.instance_norm_info(4096, 1 << 20, False)).group(1))
    assert one > many
    with pytest.raises(RuntimeError):
        ops.instance_norm_info(1, 1, False)
    with pytest.raises(RuntimeError):
        ops.instance_norm_info(0, 8, False)


class _Normed(nn.Module):
    def __init__(self, affine):
        super().__init__()
        self.w = nn.Parameter(torch.randn(3)) if affine else None
        self.b = nn.Parameter(torch.randn(3)) if affine else None

    def forward(self, x):
        return ops.instance_norm(x * 2.0, self.w, self.b, 1e-6)


@pytest.mark.parametrize("affine", [True, False])
def test_instance_norm_export_round_trip(affine):
    torch.manual_seed(5)
    m, x = _Normed(affine).eval(), torch.randn(2, 3, 7, 9)
    data = ex.export(m, (x,))
    nodes = [(n.domain, n.op_type) for n in P.load_model(data).graph.node]
    assert ("com.amd.dft", "instance_norm") in nodes
    (y,) = OnnxGraph(data, torch.device("cpu")).run(x)
    with torch.no_grad():
        assert torch.equal(y, m(x))


def test_stock_instance_norm_through_the_runner():
    torch.manual_seed(6)
    m = nn.Sequential(nn.Conv2d(3, 4, 1), nn.InstanceNorm2d(4, eps=1e-6, affine=True)).eval()
    with torch.no_grad():
        m[1].weight.normal_()
        m[1].bias.normal_()
    x = torch.randn(2, 3, 7, 9)
    data = ex.export(m, (x,))
    assert ("", "InstanceNormalization") in [(n.domain, n.op_type) for n in P.load_model(data).graph.node]
    (y,) = OnnxGraph(data, torch.device("cpu")).run(x)
    with torch.no_grad():
        assert torch.allclose(y, m(x), atol=1e-5)
