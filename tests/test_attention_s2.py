"""Neighbourhood attention on the sphere, CPU tier: ``attention_s2_tables``, the ``attention_s2`` op's CPU and meta
kernels, the module's two backends, error checks and export.  The gfx950 kernel: tests/test_attention_s2_gpu.py.

The oracle is independent of the code under test: a dense boolean mask [nlat_out, nlon_out, nlat_in, nlon_in] from
the geodesic distance of every pair of points at their own longitudes, and a masked softmax over all input points
in a few lines of torch.  It never sees ``hw``."""
import math

import numpy as np
import pytest
import torch

from tensorrt_dft_plugins_amd import load_plugins
from tensorrt_dft_plugins_amd.engine import Engine
from tensorrt_dft_plugins_amd.models import NeighborhoodAttentionS2
from tensorrt_dft_plugins_amd.onnx import exporter as ex
from tensorrt_dft_plugins_amd.onnx import proto as P
from tensorrt_dft_plugins_amd.onnx.runner import OnnxGraph
from tensorrt_dft_plugins_amd.ops import attention_s2 as A
from tensorrt_dft_plugins_amd.ops.sht import colatitudes

load_plugins()
ops = torch.ops.amd_dft
EQ, LG = "equiangular", "legendre-gauss"

# (in_shape, grid_in, out_shape, grid_out, cutoff): the grids of the GPU cases
GRIDS = {
    "same": ((9, 24), EQ, (9, 24), EQ, 2 * math.pi / 8),
    "down": ((17, 64), LG, (9, 16), EQ, 2 * math.pi / 8),
    "wide": ((7, 160), EQ, (7, 160), EQ, 2 * math.pi / 6),
    "cap": ((5, 72), EQ, (5, 72), EQ, 0.9),
    "empty": ((6, 16), LG, (5, 16), EQ, 0.2),
}


def _dense_mask(ins, gi, outs, go, cut):
    """[nlat_out, nlon_out, nlat_in, nlon_in] bool: r < cutoff, each pair at its own longitudes."""
    ti, to = colatitudes(ins[0], gi)[0], colatitudes(outs[0], go)[0]
    s = ins[1] // outs[1]
    dphi = 2 * np.pi * (np.arange(ins[1])[None, :] - s * np.arange(outs[1])[:, None]) / ins[1]  # [Wo, Wi]
    z = (np.cos(to)[:, None, None, None] * np.cos(ti)[None, None, :, None]
         + np.sin(to)[:, None, None, None] * np.sin(ti)[None, None, :, None] * np.cos(dphi)[None, :, None, :])
    return torch.from_numpy(np.arccos(np.clip(z, -1.0, 1.0)) < cut)


def _dense_attention(q, k, v, mask, logw, heads, scale):
    B, C = q.shape[:2]
    d = C // heads
    qh, kh, vh = (t.reshape(B, heads, d, -1) for t in (q, k, v))
    score = scale * torch.einsum("bhcq,bhck->bhqk", qh, kh) + logw.repeat_interleave(k.shape[-1])
    score = score.masked_fill(~mask.reshape(qh.shape[-1], -1), float("-inf"))
    p = torch.nan_to_num(torch.softmax(score, dim=-1))  # an empty neighbourhood: a row of -inf, 0
    return torch.einsum("bhqk,bhck->bhcq", p, vh).reshape(q.shape)


def _inputs(name, B=2, heads=2, d=3, seed=0):
    ins, gi, outs, go, cut = GRIDS[name]
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, heads * d, *outs, generator=g, dtype=torch.float64)
    k = torch.randn(B, heads * d, *ins, generator=g, dtype=torch.float64)
    v = torch.randn(B, heads * d, *ins, generator=g, dtype=torch.float64)
    return q, k, v, A.attention_s2_table_holder(ins, outs, gi, go, cut)


@pytest.mark.parametrize("name", list(GRIDS))
def test_hw_is_the_brute_force_mask(name):
    ins, gi, outs, go, cut = GRIDS[name]
    hw, logw = A.attention_s2_tables(ins, outs, gi, go, cut)
    assert hw.dtype == np.int32 and hw.shape == (outs[0], ins[0]) and logw.dtype == np.float32
    assert hw.min() >= -1 and hw.max() <= ins[1] // 2
    off = (np.arange(ins[1])[None, :] - (ins[1] // outs[1]) * np.arange(outs[1])[:, None]) % ins[1]
    circ = np.minimum(off, ins[1] - off)  # [Wo, Wi]
    from_hw = circ[None, :, None, :] <= hw[:, None, :, None]
    assert np.array_equal(from_hw, _dense_mask(ins, gi, outs, go, cut).numpy())
    assert np.allclose(logw, np.log(colatitudes(ins[0], gi)[1]))


@pytest.mark.parametrize("name", list(GRIDS))
def test_cpu_op_and_torch_backend_match_the_dense_softmax(name):
    ins, gi, outs, go, cut = GRIDS[name]
    q, k, v, t = _inputs(name)
    want = _dense_attention(q, k, v, _dense_mask(ins, gi, outs, go, cut), t.logw64, 2, 0.7)
    got = A.attention_s2(q, k, v, t, scale=0.7, heads=2)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) < 1e-12
    m = NeighborhoodAttentionS2(6, ins, outs, 2, gi, go, cut, backend="torch")
    m.scale = 0.7
    assert float((m.attend_torch(q, k, v) - got).abs().max()) < 1e-12
    lo = A.attention_s2(q.bfloat16(), k.bfloat16(), v.bfloat16(), t, scale=0.7, heads=2)  # fp64 sums, one rounding
    ref = ops.attention_s2(q.bfloat16().double(), k.bfloat16().double(), v.bfloat16().double(), t.hw, t.logw, 2, 0.7)
    assert lo.dtype == torch.bfloat16 and torch.equal(lo, ref.bfloat16())


@pytest.mark.parametrize("name", ["same", "empty"])
def test_constant_v_comes_back_where_there_is_a_neighbour(name):
    q, k, v, t = _inputs(name)
    v = torch.full_like(v, 1.5)
    y = A.attention_s2(q, k, v, t, heads=2)
    live = torch.from_numpy((t.hw_host >= 0).any(axis=1))
    assert float((y[:, :, live] - 1.5).abs().max()) < 1e-14 and bool((y[:, :, ~live] == 0).all())
    assert int((~live).sum()) == (3 if name == "empty" else 0)


def test_meta_shapes_and_default_scale():
    q, k, v, t = _inputs("down")
    args = [a.to("meta") for a in (q.float(), k.float(), v.float(), t.hw, t.logw)]
    y = ops.attention_s2(*args, 2, 1.0)
    assert y.shape == q.shape and y.dtype == torch.float32 and y.device.type == "meta"
    out = torch.empty(q.shape, device="meta")
    assert ops.attention_s2_out(*args, 2, 1.0, out) is out
    assert torch.equal(A.attention_s2(q, k, v, t, heads=2), A.attention_s2(q, k, v, t, scale=3 ** -0.5, heads=2))
    assert "qtiles=1" in ops.attention_s2_info(2, 2, 3, 17, 64, 9, 16, False)


def test_errors():
    q, k, v, t = _inputs("down")
    with pytest.raises(TypeError, match="share one dtype"):
        A.attention_s2(q.float(), k.float(), v.to(torch.bfloat16), t, heads=2)
    with pytest.raises(RuntimeError, match="share one dtype"):
        ops.attention_s2(q.float(), k, v, t.hw, t.logw, 2, 1.0)
    with pytest.raises(ValueError, match="multiple of nlon_out"):
        A.attention_s2_tables((9, 24), (9, 16))
    with pytest.raises(ValueError, match="multiple of nlon_out"):
        NeighborhoodAttentionS2(4, (9, 24), (9, 16), 2)
    with pytest.raises(RuntimeError, match="hw must be int32"):
        ops.attention_s2(q, k, v, t.hw[:, :-1], t.logw, 2, 1.0)
    with pytest.raises(RuntimeError, match="attention_s2_out: out must be"):
        ops.attention_s2_out(q, k, v, t.hw, t.logw64, 2, 1.0, torch.empty(q.shape))


def test_export_runner_engine(tmp_path):
    ins, gi, outs, go, cut = GRIDS["down"]
    torch.manual_seed(4)
    m = NeighborhoodAttentionS2(6, ins, outs, 2, gi, go, cut, out_chans=5).eval()
    x, kv = torch.randn(2, 6, *outs), torch.randn(2, 6, *ins)
    with torch.no_grad():
        eager = m(x, kv)
        assert float((eager - m.set_backend("torch")(x.double(), kv.double())).abs().max()) < 1e-5
    m.set_backend("amd")
    data = ex.export(m, (x, kv))
    nodes = P.load_model(data).graph.node
    assert [n.op_type for n in nodes if n.domain == "com.amd.dft"] == 3 * ["fno_pointwise"] + ["attention_s2",
                                                                                                "fno_pointwise"]
    assert {n.op_type for n in nodes if n.domain != "com.amd.dft"} <= {"Constant"}
    (y,) = OnnxGraph(data, torch.device("cpu")).run(x, kv)
    assert torch.equal(y, eager)
    eng = Engine.build(m, (x, kv), device="cpu")
    path = str(tmp_path / "attention_s2.engine")
    eng.save(path)
    (yl,) = Engine.load(path, device="cpu").infer(x, kv)
    assert torch.equal(yl, eager)
