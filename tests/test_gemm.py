"""Fused-epilogue bf16 GEMM (csrc/nn/gemm.hip) vs an fp32 PyTorch reference."""
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_l2


def _ref(x, w, b, act, r):
    y = F.linear(x.float(), w.float(), None if b is None else b.float())
    if act == 1:
        y = F.gelu(y)
    if r is not None:
        y = y + r.float()
    return y


def test_linear_cpu_semantics():
    torch.manual_seed(0)
    x = torch.randn(5, 64)
    w = torch.randn(256, 64)
    b = torch.randn(256)
    r = torch.randn(5, 256)
    y = torch.ops.amd_dft.linear(x, w, b, 1, r)
    assert rel_l2(y, _ref(x, w, b, 1, r)) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,act,bias,res", [
    (1000, 3072, 768, 1, True, False),   # FourCastNet fc1 shape (fewer rows)
    (777, 768, 3072, 0, True, True),     # fc2 + residual, ragged M
    (256, 256, 64, 0, False, False),
    (300, 1280, 768, 0, True, False),    # head
    (33, 512, 128, 1, True, True),
])
def test_linear_gemm_gpu(device, M, N, K, act, bias, res):
    torch.manual_seed(M + N + K)
    x = (torch.randn(M, K) * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N) * 0.1 if bias else None
    r = torch.randn(M, N).to(torch.bfloat16) if res else None
    ref = _ref(x, w, b, act, r)
    y = torch.ops.amd_dft.linear(x.to(device), w.to(device), None if b is None else b.to(device), act,
                                 None if r is None else r.to(device))
    assert y.dtype == torch.bfloat16 and y.shape == (M, N)
    assert rel_l2(y.float().cpu(), ref) < 6e-3


@pytest.mark.gpu
def test_linear_gemm_asymmetric_exact(device):
    """Integer operands (exact in bf16/fp32): catches transposed / permuted fragment maps."""
    M, N, K = 256, 256, 128
    x = torch.randint(-2, 3, (M, K)).to(torch.bfloat16)
    w = torch.randint(-2, 3, (N, K)).to(torch.bfloat16)
    w[0, :] = 0
    w[0, 5] = 1  # y[:, 0] = x[:, 5]
    y = torch.ops.amd_dft.linear(x.to(device), w.to(device), None, 0, None).float().cpu()
    ref = x.float() @ w.float().t()
    assert torch.equal(y, ref)
    assert torch.equal(y[:, 0], x[:, 5].float())


def _ln_fold_operands(fc_w, fc_b, gamma, beta):
    wg = (fc_w.float() * gamma.float()[None, :]).to(torch.bfloat16)
    c1 = wg.float().sum(1)
    c2 = fc_w.float() @ beta.float() + fc_b.float()
    return wg, c1, c2


def _ln_stats(x, eps):
    xf = x.float()
    return torch.stack([xf.mean(-1), torch.rsqrt(xf.var(-1, unbiased=False) + eps)], -1)


def test_linear_ln_cpu_semantics():
    """linear_ln(x) == fc(LN(x)) with the fold operands (pinned to the torch composition)."""
    torch.manual_seed(1)
    M, K, N = 7, 64, 256
    x = torch.randn(M, K) * 2 + 0.7
    w, b = torch.randn(N, K) / 8, torch.randn(N)
    g, be = torch.randn(K) * 0.2 + 1, torch.randn(K) * 0.1
    wg, c1, c2 = _ln_fold_operands(w, b, g, be)
    y = torch.ops.amd_dft.linear_ln(x, wg, c1, c2, _ln_stats(x, 1e-6), 1)
    ref = F.gelu(F.linear(F.layer_norm(x, (K,), eps=1e-6), wg.float(), c2))  # same rounded W * gamma
    ref2 = F.gelu(F.linear(F.layer_norm(x, (K,), g, be, 1e-6), w, b))
    assert rel_l2(y, ref2) < 5e-3  # bf16-rounded W * gamma
    assert rel_l2(y, ref) < 1e-5
    with pytest.raises(RuntimeError):
        torch.ops.amd_dft.linear_ln(x, wg, c1[:-1], c2, _ln_stats(x, 1e-6), 1)


@pytest.mark.gpu
@pytest.mark.parametrize("M,act", [(1000, 1), (777, 0)])
def test_linear_ln_gpu(device, M, act):
    """LN2 folded into fc1 on the hand GEMM vs LayerNorm -> linear in fp32 (FourCastNet fc1
    shape; the residual stream carries a large mean to exercise the mean * c1 correction)."""
    torch.manual_seed(M)
    K, N = 768, 3072
    x = (torch.randn(M, K) * 1.5 + 3.0).to(torch.bfloat16)
    w, b = torch.randn(N, K) / K ** 0.5, torch.randn(N) * 0.1
    g, be = torch.randn(K) * 0.2 + 1, torch.randn(K) * 0.1
    wg, c1, c2 = _ln_fold_operands(w, b, g, be)
    st = torch.ops.amd_dft.ln_stats(x.to(device), None, 1e-6)
    y = torch.ops.amd_dft.linear_ln(x.to(device), wg.to(device), c1.to(device), c2.to(device), st, act)
    assert y.dtype == torch.bfloat16 and y.shape == (M, N)
    ref = F.linear(F.layer_norm(x.float(), (K,), g, be, 1e-6), w, b)
    if act:
        ref = F.gelu(ref)
    assert rel_l2(y.float().cpu(), ref) < 8e-3


def test_linear_gelu_tanh_cpu_semantics():
    """act = 2: GELU in the tanh form (torch's approximate="tanh"), the bf16 path's option."""
    torch.manual_seed(2)
    x, w, b = torch.randn(5, 64), torch.randn(256, 64) / 8, torch.randn(256)
    y = torch.ops.amd_dft.linear(x, w, b, 2, None)
    assert rel_l2(y, F.gelu(F.linear(x, w, b), approximate="tanh")) < 1e-6
    with pytest.raises(RuntimeError):
        torch.ops.amd_dft.linear(x, w, b, 4, None)


@pytest.mark.gpu
@pytest.mark.parametrize("ln", [False, True])
def test_linear_gelu_tanh_gpu(device, ln):
    """act = 2 on the hand GEMM (FourCastNet fc1 shape, plain and LN-folded) vs torch's tanh GELU in
    fp32, and its distance from the erf form stays below bf16 resolution."""
    torch.manual_seed(11)
    M, K, N = 1000, 768, 3072
    x = (torch.randn(M, K) * 1.5 + (3.0 if ln else 0.0)).to(torch.bfloat16)
    w, b = torch.randn(N, K) / K ** 0.5, torch.randn(N) * 0.1
    if ln:
        g, be = torch.randn(K) * 0.2 + 1, torch.randn(K) * 0.1
        wg, c1, c2 = _ln_fold_operands(w, b, g, be)
        st = torch.ops.amd_dft.ln_stats(x.to(device), None, 1e-6)
        y = torch.ops.amd_dft.linear_ln(x.to(device), wg.to(device), c1.to(device), c2.to(device), st, 2)
        pre = F.linear(F.layer_norm(x.float(), (K,), g, be, 1e-6), w, b)
    else:
        wb = w.to(torch.bfloat16)
        y = torch.ops.amd_dft.linear(x.to(device), wb.to(device), b.to(device), 2, None)
        pre = F.linear(x.float(), wb.float(), b)
    yf = y.float().cpu()
    assert rel_l2(yf, F.gelu(pre, approximate="tanh")) < 8e-3
    assert (F.gelu(pre, approximate="tanh") - F.gelu(pre)).abs().max() < 5e-4  # the form's own distance


def test_linear_gelu_erf_fit_cpu_semantics():
    """act = 3: the bf16 paths' erf GELU (x sigmoid(x q(x^2)), csrc/nn/gelu.h) is within 2.6e-5 absolute of
    the exact erf GELU over the whole line, 18x closer than the tanh form."""
    x = torch.linspace(-30, 30, 600001, dtype=torch.float64).float().reshape(-1, 1)
    w = torch.ones(64, 1)  # y[:, n] = x
    y = torch.ops.amd_dft.linear(x, w, None, 3)[:, 0].double()
    exact = torch.nn.functional.gelu(x[:, 0].double())
    assert (y - exact).abs().max() < 3e-5
    tanh = torch.nn.functional.gelu(x[:, 0].double(), approximate="tanh")
    assert (tanh - exact).abs().max() > 4e-4  # the form it replaces as the bf16 default


@pytest.mark.gpu
def test_linear_gelu_erf_fit_gpu(device):
    """act = 3 on the hand GEMM (FourCastNet fc1 shape, bf16) against the exact erf GELU of the same
    pre-activation: the epilogue's form is below bf16 resolution."""
    torch.manual_seed(3)
    M, K, N = 4096, 768, 3072
    x = torch.randn(M, K, device=device).to(torch.bfloat16)
    w = (0.03 * torch.randn(N, K, device=device)).to(torch.bfloat16)
    b = 0.1 * torch.randn(N, device=device)
    y = torch.ops.amd_dft.linear(x, w, b, 3).float()
    pre = torch.nn.functional.linear(x.float(), w.float(), b)
    ref = torch.nn.functional.gelu(pre)
    assert rel_l2(y, ref) < 4e-3  # bf16 output rounding
    yt = torch.ops.amd_dft.linear(x, w, b, 2).float()
    assert rel_l2(y, ref) <= rel_l2(yt, ref)


# ------------------------------------------------------------------ Meta and CPU implementations agree
def _meta_cases():
    """(id, op, args) for every op of csrc/ops/nn_ops.cpp: the smallest shapes the ops accept with a ragged
    256-panel (N = 128), a multi-dim leading shape and, for the patch ops, a non-square 2 x 3 patch grid."""
    bf = torch.bfloat16
    x, w, b = torch.randn(2, 3, 64), torch.randn(128, 64) / 8, torch.randn(128)
    r, pre, c1 = torch.randn(2, 3, 128), torch.randn(128), torch.randn(128)
    stats = torch.stack([torch.zeros(6), torch.ones(6)], -1)
    xs, ws = torch.ops.amd_dft.split_bf16(x, True), torch.ops.amd_dft.split_bf16(w, True)
    img = torch.randn(1, 2, 16, 24)  # C = 2, h = 2, w = 3 at p = 8: K = 128
    pw, pb, pos = torch.randn(64, 128) / 8, torch.randn(64), torch.randn(6, 64)
    pws = torch.ops.amd_dft.split_bf16(pw, True)
    uw, ub = torch.randn(64, 64) / 8, torch.randn(64)  # linear_unpatch*: C = 1, N = 64
    uws = torch.ops.amd_dft.split_bf16(uw, True)
    return [
        ("patchify", "patchify", (img, 8)),
        ("unpatchify", "unpatchify", (torch.randn(1, 2, 3, 128), 2, 2, 3, 8)),
        ("linear", "linear", (x, w, b, 1, r)),
        ("linear-bf16", "linear", (x.to(bf), w.to(bf), None, 0, None)),
        ("linear_ln", "linear_ln", (x, w, c1, b, stats, 1)),
        ("patch_linear", "patch_linear", (img, pw, pb, pos, 8)),
        ("linear_unpatch", "linear_unpatch", (x, uw, ub, 1, 2, 3, 8)),
        ("split_bf16-rows", "split_bf16", (x, True)),
        ("split_bf16-planes", "split_bf16", (x, False)),
        ("linear3", "linear3", (xs, ws, b, 1, r, False)),
        ("linear3-split_out", "linear3", (xs, ws, b, 1, None, True)),
        ("linear3_stats", "linear3_stats", (xs, ws, r, pre)),
        ("linear3_stats_pr", "linear3_stats_pr", (xs, ws, torch.ops.amd_dft.split_bf16(r.reshape(6, 128), True), stats,
                                                  pre, torch.zeros(6, 128, dtype=bf))),
        ("linear_stats", "linear_stats", (x.to(bf), w.to(bf), r.to(bf), pre)),
        ("linear3_ln", "linear3_ln", (xs, ws, c1, b, stats, 1)),
        ("patch_linear3-planes", "patch_linear3", (torch.ops.amd_dft.split_bf16(img, False), pws, pb, pos, 8)),
        ("patch_linear3-raw", "patch_linear3", (img, pws, pb, pos, 8)),
        ("linear_unpatch3", "linear_unpatch3", (xs, uws, ub, 1, 2, 3, 8)),
    ]


_META_IDS = ["patchify", "unpatchify", "linear", "linear-bf16", "linear_ln", "patch_linear", "linear_unpatch",
             "split_bf16-rows", "split_bf16-planes", "linear3", "linear3-split_out", "linear3_stats", "linear3_stats_pr",
             "linear_stats", "linear3_ln", "patch_linear3-planes", "patch_linear3-raw", "linear_unpatch3"]


@pytest.mark.parametrize("case", _META_IDS)
def test_nn_ops_meta_matches_cpu(case):
    """Every op's Meta kernel reports the shapes and dtypes its CPU kernel returns (tuples element by element)."""
    torch.manual_seed(0)
    cases = _meta_cases()
    assert [c[0] for c in cases] == _META_IDS
    assert {c[1] for c in cases} == {
        "patchify", "unpatchify", "linear", "linear_ln", "patch_linear", "linear_unpatch", "split_bf16", "linear3",
        "linear3_stats", "linear3_stats_pr", "linear_stats", "linear3_ln", "patch_linear3", "linear_unpatch3"}
    _, name, args = cases[_META_IDS.index(case)]
    op = getattr(torch.ops.amd_dft, name)
    got = op(*args)
    meta = op(*[a.to("meta") if isinstance(a, torch.Tensor) else a for a in args])
    got, meta = (got, meta) if isinstance(got, tuple) else ((got,), (meta,))
    assert len(got) == len(meta)
    for g, m in zip(got, meta):
        assert m.device.type == "meta"
        assert m.shape == g.shape and m.dtype == g.dtype


# ------------------------------------------------------------------ operand normalisation
def _strided(t):
    """A buffer twice as wide whose every other column holds t: buf[..., ::2] is t as a non-contiguous view."""
    buf = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype)
    buf[..., ::2] = t
    return buf


def _normalisation_outputs(dev, strided):
    """linear / linear_stats / linear3 / linear3_stats at M=300, N=256, K=64 on ``dev``.  ``strided``: x and the
    residual arrive as non-contiguous views and bias / pre as bf16 (the same, bf16-representable, values)."""
    ops = torch.ops.amd_dft
    bf = torch.bfloat16
    torch.manual_seed(5)
    M, N, K = 300, 256, 64
    x, w, r = (torch.randn(M, K) * 0.5).to(bf), (torch.randn(N, K) / 8).to(bf), torch.randn(M, N).to(bf)
    xs, ws = ops.split_bf16(torch.randn(M, K) * 0.5, True), ops.split_bf16(torch.randn(N, K) / 8, True)
    rf = torch.randn(M, N)
    b, pre = (torch.randn(N) * 0.1).to(bf), (torch.randn(N) * 0.1).to(bf)

    def view(t):
        if not strided:
            return t.to(dev)
        v = _strided(t).to(dev)[..., ::2]
        assert not v.is_contiguous() and torch.equal(v.cpu(), t)
        return v

    def vec(t):
        return t.to(dev) if strided else t.float().to(dev)

    w, ws = w.to(dev), ws.to(dev)
    out = [ops.linear(view(x), w, vec(b), 1, view(r))]
    out += ops.linear_stats(view(x), w, view(r), vec(pre))
    out += [ops.linear3(view(xs), ws, vec(b), 0, view(rf), False)]
    out += ops.linear3_stats(view(xs), ws, view(rf), vec(pre))
    return out


@pytest.mark.gpu
def test_operand_normalisation_reaches_kernel_unchanged(device):
    """Contiguous operands with fp32 bias / pre, and the same values as non-contiguous views with bf16 bias / pre,
    give bit-identical outputs on the hand GEMM: the wrappers' .contiguous() / dtype conversions hand the kernel the
    same bytes (same kernel, one workgroup per tile, no atomics: no tolerance).  The CPU implementation is checked
    first, so the inputs' construction cannot be what fails."""
    from tensorrt_dft_plugins_amd.utils import strict_mode

    cpu = torch.device("cpu")
    for a, b in zip(_normalisation_outputs(cpu, False), _normalisation_outputs(cpu, True)):
        assert torch.equal(a, b)
    prev = strict_mode(True)
    try:
        plain, views = _normalisation_outputs(device, False), _normalisation_outputs(device, True)
    finally:
        strict_mode(prev)
    assert len(plain) == len(views) == 6
    for a, b in zip(plain, views):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a, b)
