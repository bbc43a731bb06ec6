"""The ``attention_s2_global`` kernel (csrc/spectral/attention_s2_global.hip) and ``AttentionS2`` on the GPU, under
``strict_mode`` with no fallback counted.  What each case of CASES can break: ``tail`` a single ragged chunk, a
partial query tile, the -inf bias tail; ``cross`` 20 % 9 != 0, d padded to 32, batch and head indexing, three chunks
with the last ragged, chunks crossing latitude rows, both LDS buffers; ``d64`` three query tiles with the last ragged
(8 queries), DP = 64; ``d128`` DP = 128, eight output row tiles; ``d80`` a ragged row tile at DP = 128.  ``tail`` and
``d64`` run again with q multiplied by 8, so the maximum moves between chunks and the rescale path is exercised.

Reference: the definition in plain torch fp64 on the same fp32 / bf16 values (not the op under test); A is the same
with |v|.  Bounds: those derived in tests/test_attention_s2_gpu.py, the arithmetic is the same: bf16
|y - ref| <= 2^-7 A; fp32 |y - ref| <= (2 eps + 2^-15) A, eps = 2^-15 scale max sum_c |q_c| |k_c| from the case's own
data.  Module: per field against the fp64 torch backend, fp32 < 1e-5, bf16 < 2e-2.

Measured on an MI355X: worst err / bound bf16 0.32 (``tail``; 0.67 with q x 8, ``d64``), fp32 0.014 (``tail``; 0.025
with q x 8); guarded ``cross`` 0.010 / 0.215; module fp32 4.1e-6 (``cross``) and 6.6e-6 (``tail``), bf16 6.9e-3 and
9.1e-3.  With the plain three-product split (no rest plane of K and V) the fp32 module measured 1.12e-5 on ``tail``."""
import re

import pytest
import torch

from test_kernel_bounds_gpu import Guarded, _check_untouched
from tensorrt_dft_plugins_amd import utils
from tensorrt_dft_plugins_amd.models import AttentionS2
from tensorrt_dft_plugins_amd.ops import attention_s2 as A
from tensorrt_dft_plugins_amd.ops import spectral as SP

ops = torch.ops.amd_dft
BF = torch.bfloat16
EQ, LG = "equiangular", "legendre-gauss"

# name -> (B, heads, d, in_shape, grid_in, out_shape, grid_out)
CASES = {
    "tail": (1, 1, 16, (5, 12), EQ, (5, 12), EQ),
    "cross": (2, 2, 8, (9, 20), LG, (6, 9), EQ),
    "d64": (1, 1, 64, (6, 40), EQ, (11, 24), EQ),
    "d128": (1, 1, 128, (4, 48), EQ, (3, 50), EQ),
    "d80": (1, 2, 80, (4, 48), EQ, (3, 50), EQ),
}
PRECS = ["fp32", "bf16"]


@pytest.fixture()
def strict():
    prev = utils.strict_mode(True)
    SP.fallback_reset()
    try:
        yield
        assert SP.fallback_counts() == {}
    finally:
        utils.strict_mode(prev)


def _dense(q, k, v, logw, H, scale):
    B, C = q.shape[:2]
    qh, kh, vh = (t.reshape(B, H, C // H, -1) for t in (q, k, v))
    score = scale * torch.einsum("bhcq,bhck->bhqk", qh, kh) + logw.repeat_interleave(k.shape[-1])
    return torch.einsum("bhqk,bhck->bhcq", torch.softmax(score, dim=-1), vh).reshape(q.shape)


_REFS = {}


def _case(name, prec, qmul=1):
    """(q, k, v on the CPU in the case's dtype, logw fp32, heads, scale, fp64 ref, fp64 A, eps), built once and left
    unchanged."""
    key = (name, prec, qmul)
    if key not in _REFS:
        B, H, d, ins, gi, outs, go = CASES[name]
        logw = torch.from_numpy(A.attention_s2_global_tables(ins, gi))
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        dt = BF if prec == "bf16" else torch.float32
        q = (qmul * torch.randn(B, H * d, *outs, generator=g)).to(dt)
        k = torch.randn(B, H * d, *ins, generator=g).to(dt)
        v = torch.randn(B, H * d, *ins, generator=g).to(dt)
        scale = d ** -0.5
        ref = _dense(q.double(), k.double(), v.double(), logw.double(), H, scale)
        mag = _dense(q.double(), k.double(), v.double().abs(), logw.double(), H, scale)
        qa, ka = q.double().abs().reshape(B, H, d, -1), k.double().abs().reshape(B, H, d, -1)
        eps = 2.0 ** -15 * scale * float(torch.einsum("bhcq,bhck->bhqk", qa, ka).max())
        _REFS[key] = (q, k, v, logw, H, scale, ref, mag, eps)
    return _REFS[key]


def _check(y, case, prec, what):
    ref, mag, eps = case[6:]
    err = (y.detach().cpu().double() - ref).abs()
    bound = (2.0 ** -7 if prec == "bf16" else 2 * eps + 2.0 ** -15) * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"MEASURED attention_s2_global {what} {prec} max |err| {float(err.max()):.3e} worst err/bound {worst:.3f}")
    assert bool((err <= bound).all())


def _run(device, case):
    q, k, v, logw, H, scale = case[:6]
    return ops.attention_s2_global(q.to(device), k.to(device), v.to(device), logw.to(device), H, scale)


def test_every_instance_is_reached_and_d64_has_three_query_tiles():
    """Host only, from ``attention_s2_global_info``."""
    seen = set()
    for name, (B, H, d, ins, _, outs, _) in CASES.items():
        for bf in (False, True):
            f = {k: int(v) for k, v in
                 re.findall(r"(\w+)=(\d+)", ops.attention_s2_global_info(B, H, d, *ins, *outs, bf))}
            nq = outs[0] * outs[1]
            assert f["qwg"] == 4 * f["qwave"] and f["qtiles"] == -(-nq // f["qwg"]), (name, f)
            assert f["wgs"] == B * H * f["qtiles"] and f["lds"] <= 163840 and f["chunk"] == 64, (name, f)
            seen.add((f["DP"], bf))
            if name == "d64":
                assert f["qtiles"] == 3 and f["qwg"] == 128 and nq % 128
    assert seen == {(dp, bf) for dp in (32, 64, 128) for bf in (False, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,qmul", [(n, 1) for n in CASES] + [("tail", 8), ("d64", 8)])
def test_attention_s2_global_elementwise(device, strict, name, qmul, prec):
    case = _case(name, prec, qmul)
    y = _run(device, case)
    assert y.dtype == case[0].dtype and y.shape == case[6].shape
    _check(y, case, prec, f"kernel {name} q x {qmul}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_attention_s2_global_out_guard_bands(device, strict, prec):
    """``attention_s2_global_out`` with q, k, v, logw and y between NaN guard bands, one element off the 16-byte
    boundary: finite, within the bound, guards and inputs bitwise unchanged."""
    case = _case("cross", prec)
    q, k, v, logw, H, scale = case[:6]
    gs = [Guarded(device, i, t, offset=1) for i, t in enumerate((q, k, v))] + [Guarded(device, 3, logw, offset=3)]
    gy = Guarded(device, 4, shape=tuple(q.shape), dtype=q.dtype, offset=1)
    assert ops.attention_s2_global_out(*(g.view for g in gs), H, scale, gy.view) is gy.view
    _check_untouched(gs, gy)
    _check(gy.view, case, prec, "guarded cross")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_attention_s2_global_bitwise_runs_and_graph_replays(device, strict, prec):
    q, k, v, logw, H, scale = _case("d64", prec)[:6]
    args = (q.to(device), k.to(device), v.to(device), logw.to(device), H, scale)
    a = ops.attention_s2_global(*args)
    assert torch.equal(ops.attention_s2_global(*args), a)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = ops.attention_s2_global(*args)
    for _ in range(3):
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, a)


@pytest.mark.gpu
def test_device_tensors_with_d_above_128_raise(device):
    q = torch.zeros(1, 129, 3, 8, device=device)
    with pytest.raises(RuntimeError, match="head dimension"):
        ops.attention_s2_global(q, q, q, torch.zeros(3, device=device), 1, 1.0)


_MODS = {}


def _module(name):
    """(module on the CPU, query and key fp32 rounded to bf16 values, fp64 torch-backend reference), built once."""
    if name not in _MODS:
        B, H, d, ins, gi, outs, go = CASES[name]
        torch.manual_seed(21)
        m = AttentionS2(H * d, ins, outs, H, gi, go, out_chans=H * d + 3).eval()
        with torch.no_grad():
            for b in (m.q_bias, m.k_bias, m.v_bias, m.proj_bias):
                b.normal_()
            x = torch.randn(B, H * d, *outs).to(BF).float()
            kv = torch.randn(B, H * d, *ins).to(BF).float()
            ref = m.set_backend("torch")(x.double(), kv.double())
        _MODS[name] = (m.set_backend("amd"), x, kv, ref)
    return _MODS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["cross", "tail"])
def test_module_vs_fp64_torch_backend(device, strict, name, prec):
    m, x, kv, ref = _module(name)
    dt = BF if prec == "bf16" else torch.float32
    m = m.to(device)
    try:
        with torch.no_grad():
            out = m(x.to(device).to(dt), kv.to(device).to(dt))
    finally:
        m.to("cpu")
    assert out.dtype == dt and out.shape == ref.shape
    o, r = out.cpu().double().flatten(2), ref.flatten(2)
    err = float(((o - r).norm(dim=2) / r.norm(dim=2)).max())
    print(f"MEASURED attention_s2_global module {name} {prec} per-field rel-L2 {err:.3e}")
    assert err < (2e-2 if prec == "bf16" else 1e-5)
