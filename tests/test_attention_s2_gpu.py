"""The ``attention_s2`` kernel (csrc/spectral/attention_s2.hip) and ``NeighborhoodAttentionS2`` on the GPU, under
``strict_mode`` with no fallback counted.  What each case of CASES can break: ``same`` a partial query tile, whole-row
polar bands, the wrap; ``down`` s = 4, d padded to 32, batch and head indexing; ``wide`` three query tiles with the
last ragged, four output row tiles, hw 24 - 36 over several key chunks; ``cap`` equator hw = 10, union 63 + 21 = 84 >
72 while 21 < 72, so a key counts twice without the cap, and d = 40, a ragged row tile; ``empty`` 3 of 5 output rows
without a neighbour (exact 0), the other two with one.  ``same`` and ``wide`` run again with q multiplied by 8, so
the maximum moves between chunks and the rescale path is exercised.

Reference: the CPU op in fp64 on the same fp32 / bf16 inputs; A is the same op with |v| in place of v.  Elementwise
bounds, derived from what the kernel does:

* bf16: |y - ref| <= 2^-7 A.  Products of two bf16 are exact in fp32; P is rounded to bf16, the sum is taken from
  the unrounded P, one rounding at the store: three terms of 2^-9.
* fp32: |y - ref| <= (2 eps + 2^-15) A, eps = 2^-15 scale max sum_c |q_c| |k_c| from the case's own data: the bf16x3
  split perturbs every score by at most eps, which moves every softmax weight by a factor within e^(+-2 eps); the
  split of P and v, the fp32 score arithmetic, the hardware exp2 and the fp32 accumulation fit 2^-15.

Module: per field against the fp64 torch backend, fp32 < 1e-5 (``fno_pointwise`` is a bf16x3 split, the bound of
tests/test_sht_gpu.py), bf16 < 2e-2 (the bound of tests/test_disco_gpu.py).

Measured on an MI355X: worst err / bound bf16 0.43 (0.69 with q x 8), fp32 0.024 (0.037 with q x 8); module fp32
8.8e-6 (``down``) and 9.1e-6 (``same``), bf16 1.2e-2 and 7.5e-3."""
import math
import re

import pytest
import torch

from test_kernel_bounds_gpu import Guarded, _check_untouched
from tensorrt_dft_plugins_amd import utils
from tensorrt_dft_plugins_amd.models import NeighborhoodAttentionS2
from tensorrt_dft_plugins_amd.ops import attention_s2 as A
from tensorrt_dft_plugins_amd.ops import spectral as SP

ops = torch.ops.amd_dft
BF = torch.bfloat16
EQ, LG = "equiangular", "legendre-gauss"

# name -> (B, heads, d, in_shape, grid_in, out_shape, grid_out, cutoff)
CASES = {
    "same": (1, 1, 16, (9, 24), EQ, (9, 24), EQ, 2 * math.pi / 8),
    "down": (2, 2, 8, (17, 64), LG, (9, 16), EQ, 2 * math.pi / 8),
    "wide": (1, 1, 64, (7, 160), EQ, (7, 160), EQ, 2 * math.pi / 6),
    "cap": (1, 2, 40, (5, 72), EQ, (5, 72), EQ, 0.9),
    "empty": (1, 1, 16, (6, 16), LG, (5, 16), EQ, 0.2),
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


_REFS = {}


def _case(name, prec, qmul=1):
    """(q, k, v on the CPU in the case's dtype, (hw, logw), heads, scale, fp64 ref, fp64 A, eps), built once and
    left unchanged."""
    key = (name, prec, qmul)
    if key not in _REFS:
        B, H, d, ins, gi, outs, go, cut = CASES[name]
        hw, logw = (torch.from_numpy(a) for a in A.attention_s2_tables(ins, outs, gi, go, cut))
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        dt = BF if prec == "bf16" else torch.float32
        q = (qmul * torch.randn(B, H * d, *outs, generator=g)).to(dt)
        k = torch.randn(B, H * d, *ins, generator=g).to(dt)
        v = torch.randn(B, H * d, *ins, generator=g).to(dt)
        scale = d ** -0.5
        ref = ops.attention_s2(q.double(), k.double(), v.double(), hw, logw, H, scale)
        mag = ops.attention_s2(q.double(), k.double(), v.double().abs(), hw, logw, H, scale)
        qa, ka = q.double().abs().reshape(B, H, d, -1), k.double().abs().reshape(B, H, d, -1)
        eps = 2.0 ** -15 * scale * float(torch.einsum("bhcq,bhck->bhqk", qa, ka).max())
        _REFS[key] = (q, k, v, (hw, logw), H, scale, ref, mag, eps)
    return _REFS[key]


def _check(y, case, prec, what):
    ref, mag, eps = case[6:]
    err = (y.detach().cpu().double() - ref).abs()
    bound = (2.0 ** -7 if prec == "bf16" else 2 * eps + 2.0 ** -15) * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"MEASURED attention_s2 {what} {prec} max |err| {float(err.max()):.3e} worst err/bound {worst:.3f}")
    assert bool((err <= bound).all())


def _run(device, case):
    q, k, v, tables, H, scale = case[:6]
    return ops.attention_s2(q.to(device), k.to(device), v.to(device), *(t.to(device) for t in tables), H, scale)


def test_wide_has_three_query_tiles_and_every_instance_is_reached():
    """Host only, from ``attention_s2_info``."""
    seen = set()
    for name, (B, H, d, ins, _, outs, _, _) in CASES.items():
        for bf in (False, True):
            f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", ops.attention_s2_info(B, H, d, *ins, *outs, bf))}
            assert f["qtiles"] == -(-outs[1] // 64) and f["wgs"] == outs[0] * B * H * f["qtiles"], (name, f)
            seen.add((f["DP"], bf))
            if name == "wide":
                assert f["qtiles"] == 3 and outs[1] % 64
    assert seen == {(32, False), (32, True), (64, False), (64, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(CASES))
def test_attention_s2_elementwise(device, strict, name, prec):
    case = _case(name, prec)
    y = _run(device, case)
    assert y.dtype == case[0].dtype and y.shape == case[6].shape
    _check(y, case, prec, f"kernel {name}")
    if name == "empty":  # rows without a neighbour: exact zeros, not small numbers
        hw = case[3][0]
        dead = (hw < 0).all(dim=1)
        assert int(dead.sum()) == 3 and bool((y.cpu()[:, :, dead] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["same", "wide"])
def test_attention_s2_rescale_path(device, strict, name, prec):
    case = _case(name, prec, qmul=8)
    _check(_run(device, case), case, prec, f"q x 8 {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_attention_s2_out_guard_bands(device, strict, prec):
    """``attention_s2_out`` with q, k, v, logw and y between NaN guard bands, one element off the 16-byte boundary:
    finite, within the bound, guards and inputs bitwise unchanged."""
    case = _case("down", prec)
    q, k, v, (hw, logw), H, scale = case[:6]
    gs = [Guarded(device, i, t, offset=1) for i, t in enumerate((q, k, v))] + [Guarded(device, 3, logw, offset=3)]
    pad = torch.full((4096,), 0x7FFFFFFF, dtype=torch.int32)
    hb = torch.cat([pad, hw.flatten(), pad]).to(device)
    gy = Guarded(device, 4, shape=tuple(q.shape), dtype=q.dtype, offset=1)
    hv = hb[4096:4096 + hw.numel()].view(hw.shape)
    assert ops.attention_s2_out(gs[0].view, gs[1].view, gs[2].view, hv, gs[3].view, H, scale, gy.view) is gy.view
    _check_untouched(gs, gy)
    assert torch.equal(hb.cpu(), torch.cat([pad, hw.flatten(), pad]))
    _check(gy.view, case, prec, "guarded down")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_attention_s2_bitwise_runs_and_graph_replays(device, strict, prec):
    q, k, v, tables, H, scale = _case("cap", prec)[:6]
    args = (q.to(device), k.to(device), v.to(device), *(t.to(device) for t in tables), H, scale)
    a = ops.attention_s2(*args)
    assert torch.equal(ops.attention_s2(*args), a)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = ops.attention_s2(*args)
    for _ in range(3):
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, a)


@pytest.mark.gpu
def test_device_tensors_with_d_above_64_raise(device):
    q = torch.zeros(1, 65, 3, 8, device=device)
    with pytest.raises(RuntimeError, match="head dimension"):
        ops.attention_s2(q, q, q, torch.zeros(3, 3, dtype=torch.int32, device=device), torch.zeros(3, device=device),
                         1, 1.0)



_MODS = {}


def _module(name):
    """(module on the CPU, query and key fp32 rounded to bf16 values, fp64 torch-backend reference), built once."""
    if name not in _MODS:
        B, H, d, ins, gi, outs, go, cut = CASES[name]
        torch.manual_seed(21)
        m = NeighborhoodAttentionS2(H * d, ins, outs, H, gi, go, cut, out_chans=H * d + 3).eval()
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
@pytest.mark.parametrize("name", ["down", "same"])
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
    print(f"MEASURED attention_s2 module {name} {prec} per-field rel-L2 {err:.3e}")
    assert err < (2e-2 if prec == "bf16" else 1e-5)
