"""LayerNorm over the channels of NCHW fields, CPU and meta tier: the ``layer_norm_nchw`` and ``fno_pointwise_ln`` CPU
kernels against the fp64 definition, the three promises of ``layer_norm_nchw_out``, the fields and routes of
``layer_norm_nchw_info``, and ``ChannelLayerNorm`` / ``PreNormMLP`` against their fp64 torch backend, exported and run
in ``OnnxGraph``.  The gfx950 kernels: tests/test_layer_norm_nchw_gpu.py."""
import re

import pytest
import torch
import torch.nn.functional as F

from tensorrt_dft_plugins_amd import load_plugins
from tensorrt_dft_plugins_amd.models import ChannelLayerNorm, PreNormMLP
from tensorrt_dft_plugins_amd.onnx import exporter as ex
from tensorrt_dft_plugins_amd.onnx import proto as P
from tensorrt_dft_plugins_amd.onnx.runner import OnnxGraph
from tensorrt_dft_plugins_amd.ops import spectral as SP

load_plugins()
ops = torch.ops.amd_dft
BF = torch.bfloat16


def ln_ref(x, w, b, eps=1e-5):
    """The definition in fp64: F.layer_norm over the permuted tensor."""
    xd = x.double().movedim(1, -1)
    y = F.layer_norm(xd, xd.shape[-1:], None if w is None else w.double(), None if b is None else b.double(), eps)
    return y.movedim(-1, 1)


def pw_ln_ref(spec, x, g, bt, eps, w, b, gelu):
    y = torch.einsum("oi,bi...->bo...", w.double(), ln_ref(x, g, bt, eps))
    if b is not None:
        y = y + b.double().reshape(1, -1, *([1] * (x.dim() - 2)))
    if spec is not None:
        y = y + spec.double()
    return F.gelu(y) if gelu else y


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (2, 3, 7, 9), (2, 5, 6)])
def test_cpu_ops_are_the_definition_rounded_once(shape, dt):
    torch.manual_seed(3)
    C = shape[1]
    x = (1000.0 + 0.1 * torch.randn(shape)).to(dt)
    g, bt = 1 + 0.5 * torch.randn(C), torch.randn(C)
    assert torch.equal(SP.layer_norm_nchw(x, g, bt), ln_ref(x, g, bt).to(dt))
    assert torch.equal(SP.layer_norm_nchw(x), ln_ref(x, None, None).to(dt))
    w, b, spec = torch.randn(4, C), torch.randn(4), torch.randn(shape[0], 4, *shape[2:]).to(dt)
    for sp, gelu in ((spec, True), (None, False)):
        got = SP.fno_pointwise_ln(sp, x, g, bt, 1e-5, w, b, gelu)
        assert got.dtype == dt and torch.equal(got, pw_ln_ref(sp, x, g, bt, 1e-5, w, b, gelu).to(dt))


def test_out_op_keeps_its_three_promises():
    torch.manual_seed(5)
    x, w, b = torch.randn(2, 3, 5, 4), torch.randn(3), torch.randn(3)
    out = torch.empty_like(x)
    assert ops.layer_norm_nchw_out(x, w, b, 1e-5, out) is out and torch.equal(out, ops.layer_norm_nchw(x, w, b, 1e-5))
    bad = [torch.empty(2, 3, 4, 4), torch.empty(2, 3, 5, 4, dtype=BF), torch.empty(2, 3, 4, 5).transpose(-1, -2),
           torch.empty(2, 3, 5, 4, device="meta")]
    for o in bad:
        with pytest.raises(RuntimeError, match="layer_norm_nchw_out: out must be"):
            ops.layer_norm_nchw_out(x, w, b, 1e-5, o)
    for dt in (torch.float32, BF):
        xm = torch.empty(2, 3, 7, 9, dtype=dt, device="meta")
        y = ops.layer_norm_nchw(xm, torch.empty(3, device="meta"), None, 1e-5)
        assert y.shape == xm.shape and y.dtype == dt and y.device.type == "meta"
        om = torch.empty_like(xm)
        assert ops.layer_norm_nchw_out(xm, None, None, 1e-5, om) is om
        y = ops.fno_pointwise_ln(None, xm, None, None, 1e-5, torch.empty(5, 3), None, True)
        assert y.shape == (2, 5, 7, 9) and y.dtype == dt and y.device.type == "meta"


def test_info_fields_and_routes():
    def info(*a):
        s = ops.layer_norm_nchw_info(*a)
        f = dict(re.findall(r"(\w+)=(\w+)", s))
        assert set(f) == {"route", "TP", "vec", "lds", "wgs"}, s
        return f, s

    for bf16 in (False, True):
        f, _ = info(2, 128, 180 * 360, bf16)
        assert f == {"route": "resident", "TP": "256", "vec": "4", "lds": "8192", "wgs": str(2 * 254)}
        f, s = info(1, 129, 180 * 360, bf16)
        assert f == {"route": "reread", "TP": "256", "vec": "4", "lds": "8192", "wgs": "254"} and "reread(L2)" in s
        assert info(1, 8, 128 * 128, bf16)[0] == {"route": "resident", "TP": "128", "vec": "2", "lds": "4096", "wgs": "128"}
        f, _ = info(1, 128, 45 * 90, bf16)  # 16 tiles of 256: the tile narrows to fill the device
        assert f == {"route": "resident", "TP": "64", "vec": "1", "lds": "2048", "wgs": "64"}
        assert info(2, 3, 63, bf16)[0]["vec"] == "1" and info(512, 3, 1023, bf16)[0]["vec"] == "1"  # P % 4 != 0


def test_modules_against_their_fp64_torch_backend_export_and_graph():
    torch.manual_seed(7)
    x = torch.randn(2, 6, 5, 8) + torch.arange(6.0).reshape(1, 6, 1, 1)
    ln = ChannelLayerNorm(6).eval()
    mlp = PreNormMLP(6, 10).eval()
    with torch.no_grad():
        for p in list(ln.parameters()) + [mlp.norm_weight, mlp.norm_bias, mlp.fc1_bias, mlp.fc2_bias]:
            p.add_(0.3 * torch.randn_like(p))
    for m, want in ((ln, ["layer_norm_nchw"]), (mlp, ["fno_pointwise_ln", "fno_pointwise"])):
        with torch.no_grad():
            eager = m.set_backend("amd")(x)
            ref = m.set_backend("torch")(x.double())
        assert ref.dtype == torch.float64 and float((eager - ref).abs().max()) < 1e-5
        data = ex.export(m.set_backend("amd"), (x,))
        nodes = P.load_model(data).graph.node
        assert [n.op_type for n in nodes if n.domain == "com.amd.dft"] == want
        assert {n.op_type for n in nodes if n.domain != "com.amd.dft"} <= {"Constant"}
        (y,) = OnnxGraph(data, torch.device("cpu")).run(x)
        assert torch.equal(y, eager)
    model = P.load_model(ex.export(ln, (x,)))
    for n in model.graph.node:
        if n.op_type == "layer_norm_nchw":
            n.op_type = "layer_norm_nchw_out"
    with pytest.raises(NotImplementedError, match="layer_norm_nchw_out"):
        OnnxGraph(model.SerializeToString(), torch.device("cpu")).run(x)
    assert ChannelLayerNorm(6, affine=False).weight is None
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ln(x.double())
