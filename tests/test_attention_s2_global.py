"""Global attention on the sphere, CPU tier: the ``attention_s2_global`` op's CPU kernel against the definition in a
few lines of torch fp64, its tie to ``attention_s2`` with a whole-sphere table, error checks and the export of
``AttentionS2``.  The gfx950 kernel: tests/test_attention_s2_global_gpu.py."""
import numpy as np
import pytest
import torch

from tensorrt_dft_plugins_amd import load_plugins
from tensorrt_dft_plugins_amd.models import AttentionS2
from tensorrt_dft_plugins_amd.onnx import exporter as ex
from tensorrt_dft_plugins_amd.onnx import proto as P
from tensorrt_dft_plugins_amd.onnx.runner import OnnxGraph
from tensorrt_dft_plugins_amd.ops import attention_s2 as A

load_plugins()
ops = torch.ops.amd_dft
EQ, LG = "equiangular", "legendre-gauss"


def dense_attention(q, k, v, logw, heads, scale):
    """The definition: softmax over all input points of scale q.k + logw[row]."""
    B, C = q.shape[:2]
    qh, kh, vh = (t.reshape(B, heads, C // heads, -1) for t in (q, k, v))
    score = scale * torch.einsum("bhcq,bhck->bhqk", qh, kh) + logw.repeat_interleave(k.shape[-1])
    return torch.einsum("bhqk,bhck->bhcq", torch.softmax(score, dim=-1), vh).reshape(q.shape)


def _inputs(ins, outs, B=2, heads=2, d=3):
    g = torch.Generator().manual_seed(5)
    return (torch.randn(B, heads * d, *outs, generator=g, dtype=torch.float64),
            torch.randn(B, heads * d, *ins, generator=g, dtype=torch.float64),
            torch.randn(B, heads * d, *ins, generator=g, dtype=torch.float64))


def test_cpu_op_is_the_definition_on_unrelated_grids():
    ins, outs = (9, 20), (6, 9)  # 20 % 9 != 0
    q, k, v = _inputs(ins, outs)
    t = A.attention_s2_global_table_holder(ins, LG)
    got = A.attention_s2_global(q, k, v, t, scale=0.7, heads=2)
    want = dense_attention(q, k, v, t.logw64, 2, 0.7)
    assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=1e-12, atol=0)
    lo = A.attention_s2_global(q.bfloat16(), k.bfloat16(), v.bfloat16(), t, scale=0.7, heads=2)  # one rounding
    assert torch.equal(lo, dense_attention(q.bfloat16().double(), k.bfloat16().double(), v.bfloat16().double(),
                                           t.logw.double(), 2, 0.7).bfloat16())
    y = ops.attention_s2_global(q.float().to("meta"), k.float().to("meta"), v.float().to("meta"), t.logw.to("meta"),
                                2, 1.0)
    assert y.shape == q.shape and y.dtype == torch.float32 and y.device.type == "meta"


def test_equals_attention_s2_with_a_whole_sphere_table():
    ins, outs = (7, 24), (5, 12)
    q, k, v = _inputs(ins, outs)
    t = A.attention_s2_global_table_holder(ins, EQ)
    hw = torch.full((outs[0], ins[0]), ins[1] // 2, dtype=torch.int32)
    want = ops.attention_s2(q, k, v, hw, t.logw64, 2, 0.5)
    assert torch.allclose(ops.attention_s2_global(q, k, v, t.logw64, 2, 0.5), want, rtol=1e-12, atol=0)
    assert np.array_equal(A.attention_s2_global_tables(ins, EQ), A.attention_s2_tables(ins, outs)[1])


def test_mixed_dtypes_raise():
    q, k, v = _inputs((4, 8), (3, 5))
    t = A.attention_s2_global_table_holder((4, 8))
    with pytest.raises(TypeError, match="share one dtype"):
        A.attention_s2_global(q.float(), k.float(), v.bfloat16(), t, heads=2)
    with pytest.raises(RuntimeError, match="share one dtype"):
        ops.attention_s2_global(q.float(), k, v, t.logw, 2, 1.0)
    with pytest.raises(RuntimeError, match="logw must be float32"):
        ops.attention_s2_global(q.float(), k.float(), v.float(), t.logw64, 2, 1.0)


def test_module_export_runs_in_onnx_graph_and_out_op_is_refused():
    ins, outs = (9, 20), (6, 9)
    torch.manual_seed(4)
    m = AttentionS2(6, ins, outs, 2, LG, EQ, out_chans=5).eval()
    x, kv = torch.randn(2, 6, *outs), torch.randn(2, 6, *ins)
    with torch.no_grad():
        eager = m(x, kv)
        assert float((eager - m.set_backend("torch")(x.double(), kv.double())).abs().max()) < 1e-5
    data = ex.export(m.set_backend("amd"), (x, kv))
    nodes = P.load_model(data).graph.node
    assert [n.op_type for n in nodes if n.domain == "com.amd.dft"] == 3 * ["fno_pointwise"] + [
        "attention_s2_global", "fno_pointwise"]
    assert {n.op_type for n in nodes if n.domain != "com.amd.dft"} <= {"Constant"}
    (y,) = OnnxGraph(data, torch.device("cpu")).run(x, kv)
    assert torch.equal(y, eager)
    model = P.load_model(data)
    for n in model.graph.node:
        if n.op_type == "attention_s2_global":
            n.op_type = "attention_s2_global_out"
    with pytest.raises(NotImplementedError, match="attention_s2_global_out"):
        OnnxGraph(model.SerializeToString(), torch.device("cpu")).run(x, kv)
