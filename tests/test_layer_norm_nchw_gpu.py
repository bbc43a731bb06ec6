"""``layer_norm_nchw`` (csrc/spectral/layer_norm_nchw.hip), ``fno_pointwise_ln`` (the LN instances of
csrc/spectral/fno_pointwise_mfma.hip) and ``PreNormMLP`` on the GPU, under ``strict_mode`` with no fallback counted.

Standalone bound, the project's own (tests/test_instance_norm_gpu.py): every element against ``F.layer_norm`` over the
permuted tensor in fp64, |y - ref| <= max(4 e_aten, 2^-20 max|ref|) with e_aten the largest error of ATen's fp32 CPU
``layer_norm`` on the same input; bf16 adds 2^-8 |ref| for the one rounding.  Inputs N(0, 1) and the ill-conditioned
N(1000, 0.1^2).  Fused form and ``PreNormMLP``: rel-L2 per field (batch entry, output channel) against the fp64
definition, below 1e-5 in fp32 and 2e-2 in bf16, the limits of the ``fno_pointwise``-based modules.

MEASURED on an MI355X: fused fp32 worst field 1.0e-7 .. 1.3e-6, fused bf16 <= 1.6e-2, ``PreNormMLP`` 4.3e-6 fp32 and
4.0e-3 bf16.  The printed unfused ``fno_pointwise(layer_norm_nchw(x))`` reaches 2e-5 .. 1.1e-4 in fp32 where it takes
the bf16x3 MFMA kernel (Cin = 3, 33): the fused fp32 instances run a three-plane split and an erfc GELU instead."""
import functools
import re

import pytest
import torch

import test_kernel_bounds_gpu as KB
import test_layer_norm_nchw as CPU
from tensorrt_dft_plugins_amd import load_plugins, utils
from tensorrt_dft_plugins_amd.models import PreNormMLP
from tensorrt_dft_plugins_amd.ops import spectral as SP

load_plugins()  # the case list below asks layer_norm_nchw_info
BF = torch.bfloat16
ops = torch.ops.amd_dft
EPS = 1e-5
ids = lambda c: "x".join(map(str, c))  # noqa: E731
dts = pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])


@pytest.fixture()
def strict():
    prev = utils.strict_mode(True)
    SP.fallback_reset()
    try:
        yield
        assert SP.fallback_counts() == {}
    finally:
        utils.strict_mode(prev)


def _route(C, P=260):
    return re.search(r"route=(\w+)", ops.layer_norm_nchw_info(1, C, P, False)).group(1)


CR = max(c for c in range(1, 1025) if _route(c) == "resident")  # the largest resident channel count
FIXED = [(1, 1, 1, 2), (2, 3, 7, 9), (1, 5, 13, 24), (2, 64, 1, 257), (1, 130, 9, 40)]
CASES = FIXED + [(1, CR, 1, 260), (1, CR + 1, 1, 260)]


def test_derived_cases_hit_their_routes():
    assert _route(CR) == "resident" and _route(CR + 1) == "reread" and _route(130, 360) == "reread"


@functools.lru_cache(maxsize=None)
def _case(shape, kind, bf16):
    """(x, weight, bias, fp64 reference, e_aten), on the CPU, computed once."""
    g = torch.Generator().manual_seed(99 + len(kind) + 7 * sum(shape))
    x = torch.randn(*shape, generator=g)
    if kind == "ill":
        x = 1000.0 + 0.1 * x
    if bf16:
        x = x.to(BF)
    C = shape[1]
    w, b = 1.0 + 0.5 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = CPU.ln_ref(x, w, b, EPS)
    aten = torch.nn.functional.layer_norm(x.float().movedim(1, -1), (C,), w, b, EPS).movedim(-1, 1)
    return x, w, b, ref, float((aten.double() - ref).abs().max())


def _check(out, shape, kind, bf16, what):
    x, _, _, ref, e_aten = _case(shape, kind, bf16)
    assert out.shape == x.shape and out.dtype == x.dtype
    o = out.detach().cpu().double()
    assert torch.isfinite(o).all(), what
    bound = torch.full_like(ref, max(4.0 * e_aten, 2.0 ** -20 * float(ref.abs().max())))
    if bf16:
        bound = bound + 2.0 ** -8 * ref.abs()
    diff = (o - ref).abs()
    print(f"MEASURED layer_norm_nchw {what} {shape} {kind} {'bf16' if bf16 else 'fp32'} max err {float(diff.max()):.3e} "
          f"e_aten {e_aten:.3e} worst err / bound {float((diff / bound).max()):.3f}")
    assert torch.all(diff <= bound), what


@pytest.mark.gpu
@dts
@pytest.mark.parametrize("kind", ["normal", "ill"])
@pytest.mark.parametrize("shape", CASES, ids=ids)
def test_layer_norm_nchw_against_fp64(device, strict, shape, kind, bf16):
    x, w, b, _, _ = _case(shape, kind, bf16)
    xd, wd, bd = x.to(device), w.to(device), b.to(device)
    out = ops.layer_norm_nchw(xd, wd, bd, EPS)
    _check(out, shape, kind, bf16, "op")
    assert torch.equal(xd.cpu(), x)
    if shape[1] == 1:  # one channel: x - mean = 0 exactly, the result is exactly bias
        assert torch.equal(out, bd.to(x.dtype).reshape(1, 1, 1, 1).expand(shape))


@pytest.mark.gpu
@dts
@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (2, 64, 1, 257), (1, CR + 1, 1, 260)], ids=ids)
def test_layer_norm_nchw_contracts(device, strict, shape, bf16):
    """An ``_out`` call inside guard bands with NaN poison written over them: the bands of every tensor keep their
    bits, the inputs are unchanged and the result is within the bound; a view at an odd element offset, a second run
    and two hipGraph replays all equal the contiguous eager call bit for bit."""
    x, w, b, _, _ = _case(shape, "ill", bf16)
    guards = [KB.Guarded(device, 0, x), KB.Guarded(device, 1, w), KB.Guarded(device, 2, b),
              KB.Guarded(device, 3, shape=shape, dtype=x.dtype)]
    for g in guards:
        full = g.bits.view(g.view.dtype)
        full[:g.lo] = float("nan")
        full[g.hi:] = float("nan")
    before = [g.bits.clone() for g in guards]
    gx, gw, gb, go = guards
    assert ops.layer_norm_nchw_out(gx.view, gw.view, gb.view, EPS, go.view).data_ptr() == go.view.data_ptr()
    torch.cuda.synchronize()
    for g, b0 in zip(guards, before):
        assert torch.equal(g.bits[:g.lo], b0[:g.lo]) and torch.equal(g.bits[g.hi:], b0[g.hi:])
    assert gx.unchanged() and gw.unchanged() and gb.unchanged()
    _check(go.view, shape, "ill", bf16, "out in guard bands")

    xd, wd, bd = x.to(device), w.to(device), b.to(device)
    want = ops.layer_norm_nchw(xd, wd, bd, EPS)
    assert torch.equal(go.view, want) and torch.equal(ops.layer_norm_nchw(xd, wd, bd, EPS), want)
    buf = torch.zeros(xd.numel() + 8, dtype=xd.dtype, device=device)
    for off in (1, 3):
        view = buf[off:off + xd.numel()].view(shape)
        view.copy_(xd)
        assert view.data_ptr() % 16 != 0
        assert torch.equal(ops.layer_norm_nchw(view, wd, bd, EPS), want)
        out = torch.empty_like(buf)[off:off + xd.numel()].view(shape)
        assert torch.equal(ops.layer_norm_nchw_out(xd, wd, bd, EPS, out), want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.layer_norm_nchw(xd, wd, bd, EPS)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, want)


# ------------------------------------------------------------------------------------------------ fno_pointwise_ln
PW_CASES = [(3, 5, 63), (20, 40, 312), (33, 70, 260), (64, 64, 256)]
FLAGS = {"plain": (False, False, False), "all": (True, True, True), "spec": (True, False, True),
         "gelu": (False, True, False)}  # spec, gelu, affine
TOL = {False: 1e-5, True: 2e-2}


@functools.lru_cache(maxsize=None)
def _pw_case(cin, cout, P, bf16):
    g = torch.Generator().manual_seed(5 + cin + 3 * cout + P)
    dt = BF if bf16 else torch.float32
    x = (torch.randn(2, cin, P, generator=g) + 3.0 * torch.randn(cin, generator=g)[None, :, None]).to(dt)
    spec = torch.randn(2, cout, P, generator=g).to(dt)
    gamma, beta = 1.0 + 0.5 * torch.randn(cin, generator=g), torch.randn(cin, generator=g)
    w, b = torch.randn(cout, cin, generator=g) / cin ** 0.5, torch.randn(cout, generator=g)
    return x, spec, gamma, beta, w, b


def _field_err(out, ref):
    o, r = out.detach().cpu().double().flatten(2), ref.flatten(2)
    return float(((o - r).norm(dim=-1) / r.norm(dim=-1)).max())


@pytest.mark.gpu
@dts
@pytest.mark.parametrize("flags", FLAGS, ids=list(FLAGS))
@pytest.mark.parametrize("case", PW_CASES, ids=ids)
def test_fno_pointwise_ln_against_fp64(device, strict, case, flags, bf16):
    use_spec, gelu, affine = FLAGS[flags]
    x, spec, gamma, beta, w, b = _pw_case(*case, bf16)
    sp, ga, be = (spec if use_spec else None), (gamma if affine else None), (beta if affine else None)
    ref = CPU.pw_ln_ref(sp, x, ga, be, EPS, w, b, gelu)
    dev = lambda t: None if t is None else t.to(device)  # noqa: E731
    out = ops.fno_pointwise_ln(dev(sp), dev(x), dev(ga), dev(be), EPS, dev(w), dev(b), gelu)
    assert out.dtype == x.dtype and out.shape == ref.shape
    unfused = ops.fno_pointwise(dev(sp), ops.layer_norm_nchw(dev(x), dev(ga), dev(be), EPS), dev(w), dev(b), gelu)
    err = _field_err(out, ref)
    print(f"MEASURED fno_pointwise_ln {case} {flags} {'bf16' if bf16 else 'fp32'} worst field rel-L2 {err:.3e} "
          f"(unfused {_field_err(unfused, ref):.3e}) max |fused - unfused| {float((out - unfused).abs().max()):.3e}")
    assert err < TOL[bf16]
    assert torch.equal(ops.fno_pointwise_ln(dev(sp), dev(x), dev(ga), dev(be), EPS, dev(w), dev(b), gelu), out)


@pytest.mark.gpu
@dts
def test_fno_pointwise_ln_guard_bands(device, strict, bf16):
    """33 -> 70 at P = 260 (a ragged second slab, a second output group, a ragged pixel tile): x and spec inside
    guard bands of NaN.  The bands and the inputs keep their bits and no NaN reaches y, which is finite, within the
    limit and equal to the call on plain tensors.  (The fused op has no ``_out`` form, so y itself has no bands.)"""
    x, spec, gamma, beta, w, b = _pw_case(33, 70, 260, bf16)
    gx, gs = KB.Guarded(device, 0, x), KB.Guarded(device, 1, spec)
    out = ops.fno_pointwise_ln(gs.view, gx.view, gamma.to(device), beta.to(device), EPS, w.to(device), b.to(device), True)
    torch.cuda.synchronize()
    assert gx.guards_intact() and gx.unchanged() and gs.guards_intact() and gs.unchanged()
    assert torch.isfinite(out.float()).all()
    assert _field_err(out, CPU.pw_ln_ref(spec, x, gamma, beta, EPS, w, b, True)) < TOL[bf16]
    assert torch.equal(out, ops.fno_pointwise_ln(spec.to(device), x.to(device), gamma.to(device), beta.to(device), EPS,
                                                 w.to(device), b.to(device), True))


@pytest.mark.gpu
@dts
@pytest.mark.parametrize("case", [(40, 96, 13, 24), (64, 128, 9, 40)], ids=ids)
def test_pre_norm_mlp_against_its_fp64_torch_backend(device, strict, case, bf16):
    embed, hidden, H, W = case
    torch.manual_seed(embed)
    m = PreNormMLP(embed, hidden).eval()
    with torch.no_grad():
        for p in (m.norm_weight, m.norm_bias, m.fc1_bias, m.fc2_bias):
            p.add_(0.3 * torch.randn_like(p))
    h = (torch.randn(2, embed, H, W) + 2.0 * torch.randn(1, embed, 1, 1)).to(BF if bf16 else torch.float32)
    with torch.no_grad():
        ref = m.set_backend("torch")(h.double())
        out = m.set_backend("amd").to(device)(h.to(device))
    err = _field_err(out, ref)
    print(f"MEASURED PreNormMLP {case} {'bf16' if bf16 else 'fp32'} worst field rel-L2 {err:.3e}")
    assert out.dtype == h.dtype and err < TOL[bf16]
