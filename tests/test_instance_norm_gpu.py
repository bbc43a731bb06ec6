"""The ``instance_norm`` kernels on the GPU (csrc/spectral/instance_norm.hip), under ``strict_mode`` with no fallback
counted.

Cases: fixed shapes (a 2-element plane, P = 63 with unaligned plane bases, one and several workgroups, odd P) and
shapes derived from ``instance_norm_info``: P exactly at the resident bound and one above it (whose last chunk is a
single element), a split call with S >= 2 and a ragged, unaligned last chunk, a split call with one plane, and a split
call whose chunk is not the smallest.  Each derived case asserts the route it meant to hit.

Bound, fp32, every element against ``F.instance_norm`` in fp64: |out - ref| <= max(4 e_aten, 2^-20 max|ref|), with
e_aten the largest error of ATen's fp32 CPU ``instance_norm`` on the same input (the 4 allows for another summation
order; the floor is a handful of fp32 roundings for the subtract, rsqrt, scale and shift).  Inputs: N(0, 1) and the
ill-conditioned N(1000, 0.1^2), where E[x^2] - E[x]^2 in fp32 is wrong by hundreds.  bf16: the same reference on the
bf16 inputs plus 2^-8 |ref| for the one rounding.  ``instance_norm_stats``: the mean within the same bound relative
to the plane's std, rstd within 2^-20 plus the same term, relative.

Contracts: guard bands and NaN / Inf poison around every tensor of an ``_out`` call, inputs unchanged, a view at an odd
element offset equal to the contiguous call bit for bit, stale LDS, run-to-run and hipGraph-replay equality, and a
constant plane giving exactly ``bias``."""
import functools
import re

import pytest
import torch
import torch.nn.functional as F

import test_kernel_bounds_gpu as KB
from tensorrt_dft_plugins_amd import load_plugins, utils
from tensorrt_dft_plugins_amd.ops import spectral as SP

load_plugins()  # the case list below asks instance_norm_info
BF = torch.bfloat16
ops = torch.ops.amd_dft
EPS = 1e-5
ids = lambda c: "x".join(map(str, c))  # noqa: E731


@pytest.fixture()
def strict():
    prev = utils.strict_mode(True)
    SP.fallback_reset()
    try:
        yield
        assert SP.fallback_counts() == {}
    finally:
        utils.strict_mode(prev)


def _info(planes, P, bf16=False):
    s = ops.instance_norm_info(planes, P, bf16)
    f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", s)}
    f["route"] = re.search(r"route=(\w+)", s).group(1)
    return f


def _resident_bound():
    lo, hi = 2, 1 << 24  # resident at lo, split at hi
    assert _info(1, lo)["route"] == "resident" and _info(1, hi)["route"] == "split"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _info(1, mid)["route"] == "resident" else (lo, mid)
    return lo


PB = _resident_bound()
FIXED = [(1, 1, 1, 2), (2, 3, 7, 9), (1, 2, 33, 64), (3, 5, 45, 91), (1, 1, 181, 360)]
DERIVED = {
    "bound": (1, 2, 1, PB),
    "bound+1": (1, 2, 1, PB + 1),
    "ragged": (2, 3, 1, 40001),
    "one-plane": (1, 1, 7, 7143),
    "wide-chunk": (1, 205, 1, PB + 1),
}
CASES = FIXED + list(DERIVED.values())
assert all(torch.Size(c).numel() <= 4 << 20 for c in CASES)


def _P(shape):
    return torch.Size(shape[2:]).numel()


def test_derived_cases_hit_their_routes():
    for shape in FIXED:
        assert _info(shape[0] * shape[1], _P(shape))["route"] == "resident" or shape == (1, 1, 181, 360)
    assert _info(1, 181 * 360)["route"] == "split"
    for bf16 in (False, True):
        f = _info(2, PB, bf16)
        assert f["route"] == "resident" and f["S"] == 1 and f["chunk"] == PB and f["lds"] <= 64 * 1024
        f = _info(2, PB + 1, bf16)
        assert f["route"] == "split" and f["S"] >= 2 and (PB + 1) - (f["S"] - 1) * f["chunk"] == 1
        f = _info(6, 40001, bf16)
        assert f["route"] == "split" and f["S"] >= 2 and 40001 % f["chunk"] != 0 and f["wgs"] == 6 * f["S"]
        assert f["chunk"] % f["vec"] == 0 and 40001 % f["vec"] != 0  # chunk starts off the 16-byte grid
        f = _info(1, 7 * 7143, bf16)
        assert f["route"] == "split" and f["S"] >= 2 and f["wgs"] == f["S"]
        g = _info(205, PB + 1, bf16)
        assert g["route"] == "split" and g["chunk"] > f["chunk"] and g["S"] >= 2


@functools.lru_cache(maxsize=None)
def _case(shape, kind, bf16):
    """(x, weight, bias, fp64 reference, e_aten, fp64 mean, fp64 rstd), on the CPU, computed once."""
    g = torch.Generator().manual_seed(1234 + len(kind) + 7 * sum(shape))
    x = torch.randn(*shape, generator=g)
    if kind == "ill":
        x = 1000.0 + 0.1 * x
    if bf16:
        x = x.to(BF)
    C = shape[1]
    w = 1.0 + 0.5 * torch.randn(C, generator=g)
    b = torch.randn(C, generator=g)
    xd = x.double()
    ref = F.instance_norm(xd, weight=w.double(), bias=b.double(), eps=EPS)
    aten = F.instance_norm(x.float(), weight=w, bias=b, eps=EPS)
    e_aten = float((aten.double() - ref).abs().max())
    flat = xd.reshape(shape[0], C, -1)
    mean = flat.mean(-1)
    rstd = (flat.var(-1, unbiased=False) + EPS).rsqrt()
    return x, w, b, ref, e_aten, mean, rstd


def _bound(ref, e_aten, bf16):
    bound = torch.full_like(ref, max(4.0 * e_aten, 2.0 ** -20 * float(ref.abs().max())))
    return bound + 2.0 ** -8 * ref.abs() if bf16 else bound


def _check(out, shape, kind, bf16, what):
    x, _, _, ref, e_aten, _, _ = _case(shape, kind, bf16)
    assert out.shape == x.shape and out.dtype == x.dtype
    o = out.detach().cpu().double()
    assert torch.isfinite(o).all(), what
    diff, bound = (o - ref).abs(), _bound(ref, e_aten, bf16)
    print(f"MEASURED instance_norm {what} {shape} {kind} {'bf16' if bf16 else 'fp32'} max err {float(diff.max()):.3e} "
          f"e_aten {e_aten:.3e} worst err / bound {float((diff / bound).max()):.3f}")
    assert torch.all(diff <= bound), what


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["normal", "ill"])
@pytest.mark.parametrize("shape", CASES, ids=ids)
def test_instance_norm_against_fp64(device, strict, shape, kind, bf16):
    x, w, b, _, _, _, _ = _case(shape, kind, bf16)
    xd, wd, bd = x.to(device), w.to(device), b.to(device)
    out = ops.instance_norm(xd, wd, bd, EPS)
    _check(out, shape, kind, bf16, "op")
    assert torch.equal(ops.instance_norm(xd, wd, bd, EPS), out)  # run to run
    assert torch.equal(xd.cpu(), x)


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["normal", "ill"])
@pytest.mark.parametrize("shape", CASES, ids=ids)
def test_instance_norm_stats(device, strict, shape, kind, bf16):
    """The bound of the output, |out - ref| <= max(4 e_aten, 2^-20 max|ref|), applied to the mean: ``ref`` is the
    fp64 mean, and the e_aten term, which is in units of the normalised output, is taken relative to the plane's std:
    |mean - ref| <= max(4 e_aten std, 2^-20 max|ref mean|).  The floor is what it is for the output, a handful of fp32
    roundings of the quantity compared -- here the mean itself, which an fp32 result holds to half an ulp, 2^-24 of
    its size, at best.  (An earlier version of this test took max|ref| from the normalised output instead, a floor
    of a few 1e-6 of the std; at N(1000, 0.1^2) the fp64 mean rounded to fp32 is already up to 3e-4 of the std away,
    so no fp32 [B, C, 2] result could meet it once e_aten happened to be small.)  rstd: relative error within 2^-20
    plus the output's term."""
    x, _, _, ref, e_aten, mean, rstd = _case(shape, kind, bf16)
    st = ops.instance_norm_stats(x.to(device), EPS)
    assert st.shape == (shape[0], shape[1], 2) and st.dtype == torch.float32
    s = st.cpu().double()
    term = max(4.0 * e_aten, 2.0 ** -20 * float(ref.abs().max()))
    d_mean = (s[..., 0] - mean).abs()
    b_mean = torch.clamp(4.0 * e_aten / rstd, min=2.0 ** -20 * float(mean.abs().max()))  # 1 / rstd: std, eps included
    e_rstd = float(((s[..., 1] - rstd).abs() / rstd).max())
    print(f"MEASURED instance_norm_stats {shape} {kind} {'bf16' if bf16 else 'fp32'} mean err / std "
          f"{float((d_mean * rstd).max()):.3e} worst mean err / bound {float((d_mean / b_mean).max()):.3f} "
          f"rstd rel err {e_rstd:.3e} bound term {term:.3e}")
    assert torch.all(d_mean <= b_mean)
    assert e_rstd <= 2.0 ** -20 + term


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("absent", ["weight", "bias", "both"])
def test_instance_norm_absent_affine(device, strict, absent, bf16):
    shape = (2, 3, 7, 9)
    x, w, b, _, _, _, _ = _case(shape, "normal", bf16)
    w = None if absent in ("weight", "both") else w
    b = None if absent in ("bias", "both") else b
    ref = F.instance_norm(x.double(), weight=None if w is None else w.double(), bias=None if b is None else b.double(),
                          eps=EPS)
    out = ops.instance_norm(x.to(device), None if w is None else w.to(device), None if b is None else b.to(device), EPS)
    tol = 2.0 ** -20 * float(ref.abs().max()) + (2.0 ** -8 * ref.abs() if bf16 else 0.0)
    assert torch.all((out.cpu().double() - ref).abs() <= tol)
    # per-channel arguments in x's dtype are read as fp32
    if bf16 and w is not None and b is not None:
        w16, b16 = w.to(BF), b.to(BF)
        assert torch.equal(ops.instance_norm(x.to(device), w16.to(device), b16.to(device), EPS),
                           ops.instance_norm(x.to(device), w16.float().to(device), b16.float().to(device), EPS))


GUARD_CASES = [(2, 3, 7, 9), DERIVED["bound"], DERIVED["bound+1"], DERIVED["ragged"]]


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [None, float("nan"), float("inf")], ids=["pattern", "nan", "inf"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", GUARD_CASES, ids=ids)
def test_instance_norm_guard_bands(device, strict, shape, bf16, poison):
    """An ``_out`` call inside guard bands: the bands of x, weight, bias and out keep their bits, the inputs are
    unchanged, every element of out is written and none carries the bands' NaN (or the NaN / Inf written over
    them)."""
    x, w, b, _, _, _, _ = _case(shape, "ill", bf16)
    gx = KB.Guarded(device, 0, x)
    gw, gb = KB.Guarded(device, 1, w), KB.Guarded(device, 2, b)
    go = KB.Guarded(device, 3, shape=shape, dtype=x.dtype)
    guards = [gx, gw, gb, go]
    if poison is not None:
        for g in guards:
            full = g.bits.view(g.view.dtype)
            full[:g.lo] = poison
            full[g.hi:] = poison
        before = [g.bits.clone() for g in guards]
    assert go.view.data_ptr() % 16 == 0 and gx.view.data_ptr() % 16 == 0
    ret = ops.instance_norm_out(gx.view, gw.view, gb.view, EPS, go.view)
    torch.cuda.synchronize()
    assert ret.data_ptr() == go.view.data_ptr()
    if poison is None:
        KB._check_untouched([gx, gw, gb], go)
    else:
        for g, b0 in zip(guards, before):
            assert torch.equal(g.bits[:g.lo], b0[:g.lo]) and torch.equal(g.bits[g.hi:], b0[g.hi:])
        for g in (gx, gw, gb):
            assert g.unchanged()
    _check(go.view, shape, "ill", bf16, "out in guard bands")
    assert torch.equal(go.view, ops.instance_norm(x.to(device), w.to(device), b.to(device), EPS))


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 3, 7, 9), DERIVED["ragged"]], ids=ids)
def test_instance_norm_odd_offset_view_is_copied(device, strict, shape, bf16):
    x, w, b, _, _, _, _ = _case(shape, "normal", bf16)
    xd, wd, bd = x.to(device), w.to(device), b.to(device)
    want = ops.instance_norm(xd, wd, bd, EPS)
    buf = torch.zeros(xd.numel() + 8, dtype=xd.dtype, device=device)
    for off in (1, 3):
        view = buf[off:off + xd.numel()].view(shape)
        view.copy_(xd)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        assert torch.equal(ops.instance_norm(view, wd, bd, EPS), want)
        assert torch.equal(ops.instance_norm_stats(view, EPS), ops.instance_norm_stats(xd, EPS))
        with pytest.raises(RuntimeError, match="16-byte"):
            ops.instance_norm_out(xd, wd, bd, EPS, torch.empty_like(buf)[off:off + xd.numel()].view(shape))
    # a non-contiguous x (the same elements in the same order, rows 3 elements apart in memory) is copied too
    wide = torch.zeros(*shape[:-1], shape[-1] + 3, dtype=xd.dtype, device=device)
    strided = wide[..., :shape[-1]]
    strided.copy_(xd)
    assert not strided.is_contiguous()
    assert torch.equal(ops.instance_norm(strided, wd, bd, EPS), want)


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 3, 7, 9), DERIVED["bound"], DERIVED["ragged"]], ids=ids)
def test_instance_norm_stale_lds(device, strict, shape, bf16):
    x, w, b, _, _, _, _ = _case(shape, "normal", bf16)
    xd, wd, bd = x.to(device), w.to(device), b.to(device)
    want, want_st = ops.instance_norm(xd, wd, bd, EPS), ops.instance_norm_stats(xd, EPS)
    torch.cuda.synchronize()
    ops.lds_poison()
    got = ops.instance_norm(xd, wd, bd, EPS)
    ops.lds_poison()
    got_st = ops.instance_norm_stats(xd, EPS)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(got_st, want_st)


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 5, 45, 91), DERIVED["ragged"]], ids=ids)
def test_instance_norm_graph_replay(device, strict, shape, bf16):
    x, w, b, _, _, _, _ = _case(shape, "ill", bf16)
    xd, wd, bd = x.to(device), w.to(device), b.to(device)
    eager = ops.instance_norm(xd, wd, bd, EPS).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = ops.instance_norm(xd, wd, bd, EPS)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 3, 7, 9), DERIVED["bound"], DERIVED["ragged"]], ids=ids)
def test_instance_norm_constant_plane_gives_bias(device, strict, shape, bf16):
    """A constant plane has x - mean = 0 exactly, whatever the constant: the result is exactly ``bias`` (0 without)."""
    C = shape[1]
    dt = BF if bf16 else torch.float32
    vals = torch.tensor([0.1, -1234.567, 3.0e-5, 7.0e8])[torch.arange(shape[0] * C) % 4].reshape(shape[0], C, 1, 1)
    x = vals.expand(shape).to(dt).contiguous().to(device)
    w = torch.linspace(0.5, 2.0, C, device=device)
    b = torch.linspace(-1.0, 1.0, C, device=device)
    out = ops.instance_norm(x, w, b, EPS)
    assert torch.equal(out, b.to(dt).reshape(1, C, 1, 1).expand(shape))
    assert torch.equal(ops.instance_norm(x, w, None, EPS), torch.zeros_like(x))
    st = ops.instance_norm_stats(x, EPS)
    assert torch.equal(st[..., 0], x[:, :, 0, 0].float())
