"""The hand GEMM (csrc/nn/gemm.hip) element by element at its tile, panel and K-tile edges, through the public ops,
under ``strict_mode`` with no fallback counted.  Host-only tier: the sensitivity test, the dispatch-coverage test
and the refusal checks of the CPU ops.

Reference: the sum the kernel is meant to compute, in fp64 on the CPU, from the exact operand values it multiplies.
bf16: ``sum_k x w`` from the bf16 values.  bf16x3: the three products the kernel forms,
``sum_k (x_hi w_hi + x_lo w_hi + x_hi w_lo)`` with hi / lo taken from ``split_bf16``'s k32-interleaved pairs (the
dropped ``lo * lo`` is the design's error, not the kernel's, and stays with the 2e-5 checks against the true fp32
product in tests/test_fp32_path.py).

Bounds, per element, u = 2^-24:

* accumulation: ``E_acc = c n_t u S``, ``S = sum_k |x| |w|`` over the same products, ``n_t = K`` (bf16) or ``3 K``
  (bf16x3): every product of two bf16 values is exact in fp32, and a sum of n_t terms in ANY order is within
  (n_t - 1) u S of the exact one.  ``c = 1.01`` (the IEEE value, as tests/test_disco_gpu.py); worst measured
  err / bound per form on MI355X: see "Measured" below.
* bias add: one rounding of the sum, ``u (|pre| + |bias|)``.
* LayerNorm fold ``rstd (acc - mean c1) + c2``, evaluated as fma(rstd, acc, fma(-rstd mean, c1, c2)):
  ``|rstd| (E_acc + 2 u (|acc| + |mean c1|))`` -- the roundings of -rstd mean, of the inner and of the outer fma are
  each u of a magnitude below |rstd| (|acc| + |mean c1|) + |c2|; the cancellation acc - mean c1 is carried by |acc| and
  |mean c1| separately, not by their difference -- plus the bias term above for c2.
* GELU (act 1 erf, 2 tanh form, 3 the fitted polynomial of ``gelu_erf_fit_ref`` in nn_ops.cpp), reference the fp64
  form of the same activation applied to the fp64 pre-activation: ``1.13 E_pre + E_form`` (|gelu'| <= 1.13).
  ``E_form`` = twice the largest |fp32 - fp64| of gelu.h's formulas evaluated in fp32 torch on the CPU over
  [-8, 8] (every case asserts its pre-activations lie inside); the factor 2 covers the hardware's 1-ulp rcp / exp2.
  Measured on the CPU (400001 points), already doubled: act 1 6.62e-07 (the A&S 7.1.26 erf fit's 1.5e-7 |x| / 2
  and the fp32 steps), act 2 1.03e-06, act 3 1.07e-06.
* residual add: ``u (|y| + |r|)``; the split-pair residual m + hi + lo (+ lo2) of ``linear3_stats_pr`` is summed in
  fp32 first: 3 more roundings of |m| + |hi| + |lo| + |lo2|.
* stores: bf16 ``2^-8 |ref|``; split pair (OUT 2) ``2^-16 |ref|`` on ``hi + lo``; fp32 nothing further.
* statistics partials (per token and 64-feature chunk; reference the fp64 (mean, M2) of w = the kernel's own stored
  outputs + pre): 64 fp32 roundings of the chunk's magnitudes.  The kernel shifts by the chunk's first value
  (d = w - w_0) and sums d and d^2 in one sweep.  With A = max |y| + |pre|, D = max |d|, S2 = sum d^2:
  mean: 63 roundings of the sum of d (sum |d| / 64 <= D), one of each d, and u A each for y + pre and for the final
  add: ``E_mean = 1.01 * 64 u (D + A / 32)``.
  M2 = S2 - S1^2 / 64: the rounding of y + pre moves it by 2 u sum |w - mean| |w| <= 128 u D A, that of d by
  128 u D^2, the 64 fma of S2 by 64 u S2, S1^2 / 64 by 2 |S1| (63 u sum |d|) / 64 + 2 u S1^2 / 64 <= 130 u S2
  (Cauchy-Schwarz), the final subtraction by u S2: ``E_M2 = 1.01 * 64 u (2 D (A + D) + 3.05 S2)``.

Memory contract, on the edge cases: every operand between NaN guard bands (finite, within the bound, bitwise equal to
the unguarded run, guards and inputs unchanged); every output element written (best effort: the GEMM ops allocate
their own output, so a block of the output's byte size is filled with NaN and freed first, and the caching allocator
hands the op that block; where ``data_ptr()`` shows it did not, the check is reported as not made -- at most one case
may end that way); stale LDS (the kernel fills its 128 KB by DMA and never zero-fills).

Measured on MI355X (one full run, every line in profiles/gemm_edges_measured.txt), worst err / bound per form over
all checks of this module: linear 0.989, linear_ln 0.981, linear_stats 0.994, patch_linear 0.991, linear_unpatch
0.977 (the bf16 forms sit at the bf16 store's half ulp, 2^-8 |ref|, which round-to-nearest attains); linear3 0.137,
linear3_ln 0.089, linear3_stats 0.017, linear3_stats_pr 0.008, patch_linear3 0.018, linear_unpatch3 0.006; the
statistics partials at most 0.023 (mean) and 0.025 (M2).  Nothing exceeds 1, so ``c`` stays at its IEEE value 1.01:
MFMA accumulation showed no excess over a chain of IEEE adds.  Output-written checks that could not be made: 0 of 76.

Left out: the eight LayerNorm-fold + residual instances of the bf16 dispatch, which no public op reaches; the opt-in
persistent and direct-epilogue variants (environment variables read once per process)."""
import itertools
import zlib
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_l2
from test_kernel_bounds_gpu import Guarded
from tensorrt_dft_plugins_amd import utils
from tensorrt_dft_plugins_amd.ops import spectral as SP

ops = torch.ops.amd_dft
BF, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
C_ACC = 1.01
GELU_RANGE = 8.0
SPLIT_FORMS = {"linear3", "linear3_ln", "linear3_stats", "linear3_stats_pr", "patch_linear3", "linear_unpatch3"}
STATS_FORMS = {"linear_stats", "linear3_stats", "linear3_stats_pr"}
BASE = (257, 320, 192)


@pytest.fixture()
def strict():
    prev = utils.strict_mode(True)
    SP.fallback_reset()
    try:
        yield
        assert SP.fallback_counts() == {}
    finally:
        utils.strict_mode(prev)


# ------------------------------------------------------------------------------------------------ activations
def _gelu64(act, x):
    if act == 1:
        return F.gelu(x)
    if act == 2:
        return F.gelu(x, approximate="tanh")
    if act == 3:  # gelu_erf_fit_ref (csrc/ops/nn_ops.cpp), same constants
        x2 = (x * x).clamp_max(64.0)
        z = x * (x2 * (x2 * 0.0010148165747523308 + -0.10677912831306458) + -2.3011176586151123)
        return x / (torch.exp2(z) + 1.0)
    return x


def _gelu32(act, x):
    """gelu.h's formulas, operation by operation, in fp32 torch (no fma: one more rounding per step)."""
    t = lambda v: torch.tensor(v, dtype=F32)
    if act == 1:
        ax = x.abs().clamp_max(1e30)
        r = 1.0 / (t(0.3275911 * 0.70710678118654752) * ax + 1.0)
        p = t(0.5 * 1.061405429) * r + t(0.5 * -1.453152027)
        p = p * r + t(0.5 * 1.421413741)
        p = p * r + t(0.5 * -0.284496736)
        p = p * r + t(0.5 * 0.254829592)
        p = p * r
        ex = torch.exp2((x * x) * t(-0.5 * 1.4426950408889634))
        return (-ax * p) * ex + x.clamp_min(0.0)
    if act == 2:
        c1 = t(-1.5957691216057308 * 1.4426950408889634)
        c2 = t(float(c1) * 0.044715)
        z = x * (c2 * (x * x) + c1)
        return x * (1.0 / (torch.exp2(z) + 1.0))
    if act == 3:
        x2 = (x * x).clamp_max(64.0)
        z = x * (x2 * (x2 * t(0.0010148165747523308) + t(-0.10677912831306458)) + t(-2.3011176586151123))
        return x * (1.0 / (torch.exp2(z) + 1.0))
    return x


_EFORM = {}


def _eform(act):
    """Twice the largest |fp32 evaluation - fp64 form| over [-GELU_RANGE, GELU_RANGE], measured here on the CPU."""
    if act not in _EFORM:
        x = torch.linspace(-GELU_RANGE, GELU_RANGE, 400001, dtype=torch.float64).float()
        _EFORM[act] = 2.0 * float((_gelu32(act, x).double() - _gelu64(act, x.double())).abs().max()) if act else 0.0
    return _EFORM[act]


# ------------------------------------------------------------------------------------------------ cases
def _pairs(ts):
    """k32-interleaved split rows [R, 2K] -> (hi, lo), fp64 [R, K] each."""
    p = ts.double().reshape(ts.shape[0], -1, 2, 32)
    return p[:, :, 0].reshape(ts.shape[0], -1), p[:, :, 1].reshape(ts.shape[0], -1)


def _patchify(x):
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 8, 8, W // 8, 8).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // 8) * (W // 8), C * 64)


def _unpatchify(y, B, C, h, w):
    return y.reshape(B, h, w, C, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape(B, C, h * 8, w * 8)


def _acc(prods):
    return sum(a @ b.t() for a, b in prods)


def _finish(c, acc, bias="own"):
    """The op's result in fp64 from the accumulator ``acc`` [M, N] (the reference with the exact one; the host-only
    sensitivity test feeds it subtly wrong ones)."""
    bias = c.bias64 if isinstance(bias, str) else bias
    pre = acc
    if c.ln is not None:
        mean, rstd, c1 = c.ln
        pre = rstd[:, None] * (acc - mean[:, None] * c1[None, :])
    if bias is not None:
        pre = pre + bias[None, :]
    y = _gelu64(c.act, pre)
    if c.res64 is not None:
        y = y + c.res64
    return c.post(y)


def _build(form, M, N, K, act=0, bias=False, res=False, split_out=False, rlo2=False, pos=False, grid=None):
    """One case: the op's CPU arguments in the dtypes the kernel reads, the fp64 reference and the per-element bound
    (module docstring).  ``grid`` = (B, h, w) of the patch forms (M = B h w; gather K = 64 C, scatter N = 64 C)."""
    key = (form, M, N, K, act, bias, res, split_out, rlo2, pos, grid)
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    rn = lambda *s: torch.randn(*s, generator=g)
    split = form in SPLIT_FORMS
    ln = form in ("linear_ln", "linear3_ln")
    gather, scatter = form.startswith("patch_linear"), form.startswith("linear_unpatch")
    c = SimpleNamespace(form=form, op=form, M=M, N=N, K=K, act=act, split=split, key=key, grid=grid, ln=None, res64=None,
                        bias64=None, pre=None, post=lambda y: y)
    c.name = f"{M}x{N}x{K}" + (f"-grid{'x'.join(map(str, grid))}" if grid else "") + \
        f"-a{act}b{int(bias)}r{int(res or pos)}" + ("-pair" if split_out else "") + ("-lo2" if rlo2 else "")
    if grid is not None:
        B, h, w = grid
        assert M == B * h * w
    # ---- operands and the products the kernel forms
    if gather:
        assert K % 64 == 0
        img = rn(B, K // 64, 8 * h, 8 * w) * 0.5
        xop = ops.split_bf16(img, False) if split else img.to(BF)
        xp = [_patchify(xop[0].double()), _patchify(xop[1].double())] if split else [_patchify(xop.double())]
    else:
        x = rn(M, K) * 0.5 + (1.0 if ln else 0.0)  # LN: a mean for mean * c1 to cancel
        xop = ops.split_bf16(x, True) if split else x.to(BF)
        xp = list(_pairs(xop)) if split else [xop.double()]
    wf = rn(N, K) / K ** 0.5
    wop = ops.split_bf16(wf, True) if split else wf.to(BF)
    wp = list(_pairs(wop)) if split else [wop.double()]
    c.prods = [(xp[0], wp[0])] + ([(xp[1], wp[0]), (xp[0], wp[1])] if split else [])
    c.nt = len(c.prods) * K
    b32 = rn(N) * 0.1 if bias else None
    c.bias64 = None if b32 is None else b32.double()
    res_mag, res_n = None, 0
    # ---- the op's arguments, in the dtypes the kernel reads (roles name them for the guard-band test)
    if form in ("linear", "linear3"):
        r = (rn(M, N).to(BF) if not split else rn(M, N)) if res else None
        c.args, c.roles = (xop, wop, b32, act, r) + ((split_out,) if split else ()), ("x", "w", "bias", None, "res", None)
        c.out = (2 if split_out else 1) if split else 0
    elif ln:
        xv = sum(xp)
        st = torch.stack([xv.mean(1), (xv.var(1, unbiased=False) + 1e-6).rsqrt()], 1).float()
        c1 = sum(wp).sum(1).float()
        c.ln = (st[:, 0].double(), st[:, 1].double(), c1.double())
        c.args, c.roles = (xop, wop, c1, b32, st, act), ("x", "w", "c1", "bias", "stats", None)
        c.out, r = (2 if split else 0), None
    elif form in ("linear_stats", "linear3_stats"):
        r = (rn(M, N) + 1.0) if split else (rn(M, N) + 1.0).to(BF)
        c.pre = rn(N) * 0.5
        c.args, c.roles = (xop, wop, r, c.pre), ("x", "w", "res", "pre")
        c.out = 1 if split else 0
    elif form == "linear3_stats_pr":
        rf, m = rn(M, N) * 3 + 1, rn(M) * 2
        st = torch.stack([m, torch.rand(M, generator=g) + 0.5], 1)
        rp = ops.split_bf16(rf - m[:, None], True)
        hi, lo = _pairs(rp)
        lo2 = ((rf - m[:, None]).double() - (hi + lo)).to(BF) if rlo2 else None
        l2 = lo2.double() if rlo2 else torch.zeros(M, N, dtype=torch.float64)
        c.res64 = st[:, :1].double() + hi + lo + l2
        res_mag, res_n, r = st[:, :1].double().abs() + hi.abs() + lo.abs() + l2.abs(), 3, None
        c.pre = rn(N) * 0.5
        c.args, c.roles = (xop, wop, rp, st, c.pre, lo2), ("x", "w", "rpairs", "rstats", "pre", "rlo2")
        c.out = 1
    elif gather:
        p = (rn(h * w, N) * 0.5).to(F32 if split else BF) if pos else None
        if pos:
            c.res64 = p.double().repeat(B, 1)  # row = token % (h w)
        c.args, c.roles, r = (xop, wop, b32, p, 8), ("x", "w", "bias", "pos", None), None
        c.out = 1 if split else 0
    else:
        assert scatter and N % 64 == 0
        C = N // 64
        c.args, c.roles, r = (xop, wop, b32, C, h, w, 8), ("x", "w", "bias", None, None, None, None), None
        c.out = 1 if split else 0
        c.post = lambda y: _unpatchify(y, B, C, h, w)
    if r is not None:
        c.res64 = r.double()
    c.stats = form in STATS_FORMS
    # ---- reference and bound
    acc = _acc(c.prods)
    S = sum(a.abs() @ b.abs().t() for a, b in c.prods)
    E = C_ACC * c.nt * U * S
    pre = acc
    if c.ln is not None:
        mean, rstd, c1 = c.ln
        mc1 = mean[:, None] * c1[None, :]
        E = rstd.abs()[:, None] * (E + 2 * U * (acc.abs() + mc1.abs()))
        pre = rstd[:, None] * (acc - mc1)
    if c.bias64 is not None:
        E = E + U * (pre.abs() + c.bias64.abs()[None, :])
        pre = pre + c.bias64[None, :]
    if act:
        assert float(pre.abs().max() + E.max()) < GELU_RANGE
        E = 1.13 * E + _eform(act)
    y = _gelu64(act, pre)
    if c.res64 is not None:
        if res_n:
            E = E + res_n * U * res_mag
        E = E + U * (y.abs() + (c.res64.abs() if res_mag is None else res_mag))
        y = y + c.res64
    E = E + {0: 2.0 ** -8, 1: 0.0, 2: 2.0 ** -16}[c.out] * y.abs()
    c.ref, c.bound = c.post(y), c.post(E)
    return c


_CASES = {}


def _case(*a, **k):
    """``_build`` cached (without the operand products): the reference is built once and left unchanged."""
    key = (a, tuple(sorted(k.items())))
    if key not in _CASES:
        c = _build(*a, **k)
        c.prods = None
        _CASES[key] = c
    return _CASES[key]


def _dev_args(c, device):
    return [t.to(device) if isinstance(t, torch.Tensor) else t for t in c.args]


def _run(c, args):
    return getattr(ops, c.op)(*args)


def _value(c, y):
    y = y.detach().cpu()
    if c.out == 2:
        hi, lo = _pairs(y.reshape(-1, y.shape[-1]))
        return (hi + lo).reshape(c.ref.shape)
    return y.double().reshape(c.ref.shape)


_WORST = {}


def _check(c, out, what):
    """Element by element against the case's bound; the statistics forms' partials per token and chunk."""
    y = out[0] if c.stats else out
    exp_dt = {0: BF, 1: F32, 2: BF}[c.out]
    assert y.dtype == exp_dt
    got = _value(c, y)
    assert bool(torch.isfinite(got).all())
    err = (got - c.ref).abs()
    worst = float((err / c.bound.clamp_min(1e-300)).max())
    _WORST[c.form] = max(_WORST.get(c.form, 0.0), worst)
    print(f"MEASURED gemm {c.form} {what} {c.name} max |err| {float(err.max()):.3e} rel-L2 {rel_l2(got, c.ref):.3e} "
          f"worst err/bound {worst:.3f}")
    assert bool((err <= c.bound).all()), (c.form, c.name, worst)
    if c.stats:
        _check_stats(c, y, out[1], what)
    return worst


def _stats_ref(y, pre):
    """(mean, M2, E_mean, E_M2) [M, N/64] in fp64 of w = y + pre per 64-feature chunk (module docstring)."""
    M, N = y.shape
    w = (y.double() + pre.double()[None, :]).reshape(M, N // 64, 64)
    A = (y.double().abs() + pre.double().abs()[None, :]).reshape(M, N // 64, 64).amax(2)
    mean = w.mean(2)
    m2 = (w - mean[..., None]).pow(2).sum(2)
    d = w - w[..., :1]
    D, S2 = d.abs().amax(2), d.pow(2).sum(2)
    return mean, m2, 1.01 * 64 * U * (D + A / 32), 1.01 * 64 * U * (2 * D * (A + D) + 3.05 * S2)


def _check_stats(c, y, part, what):
    assert part.dtype == F32 and tuple(part.shape) == (c.M, c.N // 64, 2)
    p = part.detach().cpu().double()
    assert bool(torch.isfinite(p).all())
    mean, m2, e_mean, e_m2 = _stats_ref(y.detach().cpu().reshape(c.M, c.N), c.pre)
    r1 = (p[..., 0] - mean).abs() / e_mean.clamp_min(1e-300)
    r2 = (p[..., 1] - m2).abs() / e_m2.clamp_min(1e-300)
    print(f"MEASURED gemm {c.form} {what} {c.name} partials max |err| mean {float((p[..., 0] - mean).abs().max()):.3e} "
          f"M2 {float((p[..., 1] - m2).abs().max()):.3e} worst err/bound mean {float(r1.max()):.3f} M2 {float(r2.max()):.3f}")
    assert bool((r1 <= 1).all()) and bool((r2 <= 1).all()), (c.form, c.name, float(r1.max()), float(r2.max()))


# ------------------------------------------------------------------------------------------------ the dispatch's leaves
# key = (MODE, SPLIT, OUT, ACT, BIAS, RES, LN, STATS) of gemm_bf16_kernel as launch_gemm instantiates it (PERSIST
# and NT aside: NT is N % 256 != 0 of the same leaf, which every token-major leaf runs too).  RES: 1 rows / pos, 2
# split pairs + shift, 3 the same + the third term.
def _leaves():
    L = []
    for act, b in itertools.product(range(4), (0, 1)):
        for r in (0, 1):
            L.append(((0, 0, 0, act, b, r, 0, 0), "linear", dict(act=act, bias=bool(b), res=bool(r))))
        L.append(((0, 0, 0, act, b, 0, 1, 0), "linear_ln", dict(act=act, bias=bool(b))))
    L.append(((0, 0, 0, 0, 0, 1, 0, 1), "linear_stats", {}))
    for act, b in itertools.product((0, 1), (0, 1)):
        for r in (0, 1):
            L.append(((0, 1, 1, act, b, r, 0, 0), "linear3", dict(act=act, bias=bool(b), res=bool(r))))
        L.append(((0, 1, 2, act, b, 0, 0, 0), "linear3", dict(act=act, bias=bool(b), split_out=True)))
        L.append(((0, 1, 2, act, b, 0, 1, 0), "linear3_ln", dict(act=act, bias=bool(b))))
    L.append(((0, 1, 2, 0, 0, 1, 0, 0), "linear3", dict(res=True, split_out=True)))
    L.append(((0, 1, 1, 0, 0, 1, 0, 1), "linear3_stats", {}))
    L.append(((0, 1, 1, 0, 0, 2, 0, 1), "linear3_stats_pr", dict(rlo2=False)))
    L.append(((0, 1, 1, 0, 0, 3, 0, 1), "linear3_stats_pr", dict(rlo2=True)))
    for s in (0, 1):
        for b, p in itertools.product((0, 1), (0, 1)):
            L.append(((1, s, s, 0, b, p, 0, 0), "patch_linear3" if s else "patch_linear", dict(bias=bool(b), pos=bool(p))))
        for b in (0, 1):
            L.append(((2, s, s, 0, b, 0, 0, 0), "linear_unpatch3" if s else "linear_unpatch", dict(bias=bool(b))))
    return L


LEAVES = _leaves()
LEAF_IDS = ["m{}s{}o{}-a{}b{}r{}-ln{}st{}".format(*k) for k, _, _ in LEAVES]


def _leaf_cases(form, flags):
    """A leaf's edge shapes: (257, 320, 192) -- a one-token last panel, a ragged 256 + 64 feature panel (NT), an odd
    bf16 K-tile count -- and, token-major, N = 256 (non-NT).  The scatter needs N % 256 == 0: C = 4."""
    M, N, K = BASE
    if form.startswith("linear_unpatch"):
        return [_build(form, M, 256, K, grid=(1, 1, M), **flags)]
    g = dict(grid=(1, 1, M)) if form.startswith("patch_linear") else {}
    return [_build(form, M, n, K, **g, **flags) for n in (N, 256)]


def test_every_dispatch_leaf_is_in_the_table_once():
    """Host only.  The expected set is spelled out from reading launch_gemm, launch_res / launch_ln / launch_split."""
    accepted = set()
    # bf16 token-major (launch_res -> launch_ln): act 0..3 x bias x residual, LayerNorm fold off ...
    accepted |= {(0, 0, 0, a, b, r, 0, 0) for a in (0, 1, 2, 3) for b in (0, 1) for r in (0, 1)}
    # ... and on.  launch_ln also accepts the fold WITH a residual (8 instances): no op passes both (linear_ln has no
    # residual argument), so they cannot be reached through the public ops and are listed as left out
    accepted |= {(0, 0, 0, a, b, 0, 1, 0) for a in (0, 1, 2, 3) for b in (0, 1)}
    unreachable = {(0, 0, 0, a, b, 1, 1, 0) for a in (0, 1, 2, 3) for b in (0, 1)}
    accepted |= {(0, 0, 0, 0, 0, 1, 0, 1)}  # linear_stats: residual, no act / bias / fold
    # bf16x3 (launch_split): fp32 out act 0/1 x bias x residual; pair out act x bias; pair out + residual alone;
    # fold (pair out, no residual) act x bias; statistics with the three residual forms
    accepted |= {(0, 1, 1, a, b, r, 0, 0) for a in (0, 1) for b in (0, 1) for r in (0, 1)}
    accepted |= {(0, 1, 2, a, b, 0, 0, 0) for a in (0, 1) for b in (0, 1)}
    accepted |= {(0, 1, 2, 0, 0, 1, 0, 0)}
    accepted |= {(0, 1, 2, a, b, 0, 1, 0) for a in (0, 1) for b in (0, 1)}
    accepted |= {(0, 1, 1, 0, 0, 1, 0, 1), (0, 1, 1, 0, 0, 2, 0, 1), (0, 1, 1, 0, 0, 3, 0, 1)}
    # gather: bias x pos, both precisions; scatter: bias, no residual
    accepted |= {(1, s, s, 0, b, r, 0, 0) for s in (0, 1) for b in (0, 1) for r in (0, 1)}
    accepted |= {(2, s, s, 0, b, 0, 0, 0) for s in (0, 1) for b in (0, 1)}
    assert len(accepted) == 57 and not (accepted & unreachable)
    refused = set()
    refused |= {(0, 1, o, a, b, r, 0, 0) for o in (1, 2) for a in (2, 3) for b in (0, 1) for r in (0, 1)}  # x3: act <= 1
    refused |= {(0, 1, 2, a, b, 1, 0, 0) for a in (0, 1) for b in (0, 1)} - {(0, 1, 2, 0, 0, 1, 0, 0)}
    refused |= {(0, 1, 2, a, b, 1, 1, 0) for a in (0, 1) for b in (0, 1)}   # split fold takes no residual
    refused |= {(0, 1, 1, a, b, r, 1, 0) for a in (0, 1) for b in (0, 1) for r in (0, 1)}  # split fold writes pairs
    refused |= {(0, s, s, a, b, 1, 0, 1) for s in (0, 1) for a in (0, 1, 2, 3) for b in (0, 1)} - accepted  # stats: plain
    refused |= {(0, s, s, 0, 0, 0, 0, 1) for s in (0, 1)}                    # statistics need the residual
    refused |= {(0, 0, 0, 0, 0, 1, 1, 1)}                                    # bf16 statistics with the fold
    refused |= {(0, 0, o, 0, 0, 0, 0, 0) for o in (1, 2)} | {(0, 1, 0, 0, 0, 0, 0, 0)}  # out != 0 <=> split
    refused |= {(m, s, s, a, 0, 0, 0, 0) for m in (1, 2) for s in (0, 1) for a in (1, 2, 3)}  # patch modes: no act
    refused |= {(2, s, s, 0, b, 1, 0, 0) for s in (0, 1) for b in (0, 1)}    # scatter: no residual
    refused |= {(1, 1, 2, 0, 0, 0, 0, 0), (2, 1, 2, 0, 0, 0, 0, 0)}          # split patch modes write fp32
    keys = [k for k, _, _ in LEAVES]
    assert len(keys) == len(set(keys)), "a leaf is in the table twice"
    assert set(keys) == accepted
    assert not (set(keys) & refused) and not (set(keys) & unreachable)
    assert len(LEAF_IDS) == len(set(LEAF_IDS))


def test_cpu_ops_refuse_what_the_dispatch_refuses():
    """Host only: the refusals the CPU ops share with the device ops (the rest need the device: K = 96 below)."""
    c = _case("linear3", 5, 64, 64, act=0, bias=True)
    xs, ws, b = c.args[0], c.args[1], c.args[2]
    for act in (2, 3, -1):
        with pytest.raises(RuntimeError, match="act must be"):
            ops.linear3(xs, ws, b, act, None, False)
    st = torch.zeros(5, 2)
    with pytest.raises(RuntimeError, match="act must be"):
        ops.linear3_ln(xs, ws, torch.zeros(64), b, st, 2)
    x, w = torch.zeros(5, 64, dtype=BF), torch.zeros(64, 64, dtype=BF)
    with pytest.raises(RuntimeError, match="act must be"):
        ops.linear(x, w, None, 4, None)
    with pytest.raises(RuntimeError, match="bias must have N"):
        ops.linear(x, w, torch.zeros(60), 0, None)
    with pytest.raises(RuntimeError, match="c1 must have N"):
        ops.linear_ln(x, w, torch.zeros(60), None, st, 0)
    with pytest.raises(RuntimeError, match="pre must have N"):
        ops.linear_stats(x, w, torch.zeros(5, 64, dtype=BF), torch.zeros(60))


# ------------------------------------------------------------------------------------------------ host-only sensitivity
def _exceeds(c, acc, bias="own"):
    return bool(((_finish(c, acc, bias) - c.ref).abs() > c.bound).any())


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
def test_bounds_catch_subtly_wrong_results(prec):
    """Host only: the bounds discriminate.  Each wrong result below, built in fp64, leaves the bound at some element,
    and the exact reference rounded to the output type stays inside it everywhere."""
    M, N, K = BASE
    split = prec == "bf16x3"
    kt = 32 if split else 64
    for flags in (dict(act=0, bias=True), dict(act=1, bias=True, res=True)) + ((dict(bias=True, split_out=True),) if split else ()):
        c = _build("linear3" if split else "linear", M, N, K, **flags)
        acc = _acc(c.prods)
        assert not _exceeds(c, acc)
        if split:  # one cross product (lo * hi) dropped in one 64 x 64 quadrant, here of the ragged half
            wrong = acc.clone()
            xl, wh = c.prods[1]
            wrong[192:256, 256:320] -= xl[192:256] @ wh[256:320].t()
            assert _exceeds(c, wrong), ("cross product", flags)
        wrong = acc - _acc([(a[:, K - kt:], b[:, K - kt:]) for a, b in c.prods])  # the last K-tile dropped
        assert _exceeds(c, wrong), ("last K-tile", flags)
        wrong = acc.clone()
        wrong[M - 1] = acc[M - 2]  # the last token row computed from row M - 2
        assert _exceeds(c, wrong), ("row M - 2", flags)
        shifted = c.bias64.clone()
        shifted[256:320] = torch.roll(c.bias64[256:320], 4)  # bias shifted by four features in the ragged half
        assert _exceeds(c, acc, shifted), ("bias shift", flags)
        # the exact reference, rounded as the kernel stores it
        if c.out == 0:
            stored = c.ref.to(BF).double()
        elif c.out == 1:
            stored = c.ref.float().double()
        else:
            stored = sum(_pairs(ops.split_bf16(c.ref.float(), True)))
        assert bool(((stored - c.ref).abs() <= c.bound).all()), flags
    # one patch row taken from the next batch image (same place in it)
    B, h, w = 3, 5, 7
    c = _build("patch_linear3" if split else "patch_linear", B * h * w, N, K, bias=True, pos=True, grid=(B, h, w))
    acc = _acc(c.prods)
    assert not _exceeds(c, acc)
    wrong = acc.clone()
    wrong[17] = acc[17 + h * w]
    assert _exceeds(c, wrong), "patch row"
    stored = c.ref.float().double() if split else c.ref.to(BF).double()
    assert bool(((stored - c.ref).abs() <= c.bound).all())
    # LayerNorm fold + fitted / erf GELU: c1 shifted by four features in the ragged half
    c = _build("linear3_ln" if split else "linear_ln", M, N, K, act=1 if split else 3, bias=True)
    acc = _acc(c.prods)
    assert not _exceeds(c, acc)
    mean, rstd, c1 = c.ln
    c1s = c1.clone()
    c1s[256:320] = torch.roll(c1[256:320], 4)
    c.ln = (mean, rstd, c1s)
    assert _exceeds(c, acc), "c1 shift"


def test_eform_values():
    """Host only: the CPU-measured E_form of the module docstring (printed; sanity window only)."""
    for act in (1, 2, 3):
        e = _eform(act)
        print(f"MEASURED gemm E_form act {act} over [-{GELU_RANGE}, {GELU_RANGE}] 2 x max |fp32 - fp64| = {e:.3e}")
        assert 0.0 < e < 1e-5


# ------------------------------------------------------------------------------------------------ every instance once
@pytest.mark.gpu
@pytest.mark.parametrize("leaf", range(len(LEAVES)), ids=LEAF_IDS)
def test_every_instance_elementwise(device, strict, leaf):
    _, form, flags = LEAVES[leaf]
    for c in _leaf_cases(form, flags):
        _check(c, _run(c, _dev_args(c, device)), "leaf")


@pytest.mark.gpu
def test_device_ops_refuse_what_the_dispatch_refuses(device, strict):
    """K = 96 is no multiple of the 64-deep K-tile: ``gemm_supported`` refuses it, so the bf16x3 ops raise and the
    bf16 op, under ``strict_mode``, raises instead of leaving the hand kernel.  The split-pair output takes a residual
    only alone; the bf16x3 ops take act 0 / 1."""
    x, w = torch.randn(257, 96), torch.randn(320, 96) / 10
    xs, ws = ops.split_bf16(x, True).to(device), ops.split_bf16(w, True).to(device)
    with pytest.raises(RuntimeError, match="K % 64 == 0"):
        ops.linear3(xs, ws, None, 0, None, False)
    with pytest.raises(RuntimeError, match="K % 64 == 0"):
        ops.linear3_stats(xs, ws, torch.zeros(257, 320, device=device), None)
    with pytest.raises(RuntimeError, match="no hand kernel"):
        ops.linear(x.to(BF).to(device), w.to(BF).to(device), None, 0, None)
    c = _case("linear3", 257, 320, 192, bias=True)
    xs, ws, b = (t.to(device) for t in c.args[:3])
    r = torch.zeros(257, 320, device=device)
    with pytest.raises(RuntimeError, match="residual only without activation and bias"):
        ops.linear3(xs, ws, b, 0, r, True)
    with pytest.raises(RuntimeError, match="residual only without activation and bias"):
        ops.linear3(xs, ws, None, 1, r, True)
    with pytest.raises(RuntimeError, match="act must be"):
        ops.linear3(xs, ws, b, 2, None, False)


# ------------------------------------------------------------------------------------------------ edge sweep
# The forms the models run: LN-folded fc1 + GELU and fc2 + residual + statistics, in bf16 and in bf16x3; the patch
# embedding; the head.
TOKEN_FORMS = {
    "fc1-bf16": ("linear_ln", dict(act=3, bias=True)),
    "fc2-bf16": ("linear_stats", {}),
    "fc1-x3": ("linear3_ln", dict(act=1, bias=True)),
    "fc2-x3": ("linear3_stats", {}),
}
# one dimension at a time around (257, 320, 192): M (the clamp at M - 1, a full tile, one token over, three token
# panels), N (one half-panel, three halves, a full panel, full + ragged, two full + ragged), K (bf16 K-tile counts 1,
# 2, 3, 5: the prologue alone, even, odd; bf16x3 2, 4, 6, 10), the one-tile and the nine-tile corners
SHAPES = [(m, 320, 192) for m in (1, 255, 256, 257, 513)] + [(257, n, 192) for n in (64, 192, 256, 576)] + \
    [(257, 320, k) for k in (64, 128, 320)] + [(256, 256, 192), (513, 576, 192)]
PATCH_GRIDS = [(3, 5, 7), (2, 9, 15)]  # M = 105: one tile across three images; M = 270: a tile edge inside an image row


def _tiles(M, N):
    return -(-M // 256) * -(-N // 256)


def test_sweep_reaches_the_edges_it_names():
    """Host only: tile counts 1, 2, 6 and 9 (the XCD remap's ``ntl % 8 != 0`` branch with q8 = 0 and q8 = 1), every
    M, N and K of the list, nothing above 513 x 576 x 320."""
    assert {_tiles(m, n) for m, n, _ in SHAPES} >= {1, 2, 6, 9}
    assert _tiles(513, 576) == 9 and 9 // 8 == 1 and 9 % 8 and all(_tiles(m, n) % 8 for m, n, _ in SHAPES)
    assert {m for m, _, _ in SHAPES} == {1, 255, 256, 257, 513} and {n for _, n, _ in SHAPES} == {64, 192, 256, 320, 576}
    assert {k for _, _, k in SHAPES} == {64, 128, 192, 320} and len(SHAPES) == len(set(SHAPES))
    assert all(m <= 513 and n <= 576 and k <= 320 for m, n, k in SHAPES)
    assert [b * h * w for b, h, w in PATCH_GRIDS] == [105, 270]


def _patch_cases():
    out = []
    for grid in PATCH_GRIDS:
        B, h, w = grid
        for form, C, N in itertools.product(("patch_linear", "patch_linear3"), (1, 3), (64, 320)):
            out.append((form, B * h * w, N, 64 * C, dict(bias=True, pos=True, grid=grid)))
        for form in ("linear_unpatch", "linear_unpatch3"):
            out.append((form, B * h * w, 256, 192, dict(bias=True, grid=grid)))
    return out


PATCH_CASES = _patch_cases()
SWEEP = [(f, m, n, k, fl) for (f, fl) in TOKEN_FORMS.values() for m, n, k in SHAPES] + PATCH_CASES
SWEEP_IDS = [f"{f}-{m}x{n}x{k}" + ("-g" + "x".join(map(str, fl["grid"])) if "grid" in fl else "") for f, m, n, k, fl in SWEEP]


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SWEEP)), ids=SWEEP_IDS)
def test_edge_sweep_elementwise(device, strict, i):
    f, m, n, k, fl = SWEEP[i]
    c = _case(f, m, n, k, **fl)
    _check(c, _run(c, _dev_args(c, device)), "sweep")


# ------------------------------------------------------------------------------------------------ memory contract
def _kernel_dtype(c, role):
    if role in ("x", "w", "rpairs", "rlo2"):
        return BF
    if role in ("res", "pos"):
        return F32 if c.split else BF
    return F32


def _same(a, b):
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    return all(x.dtype == y.dtype and torch.equal(x.view(torch.int16 if x.dtype == BF else torch.int32),
                                                    y.view(torch.int16 if y.dtype == BF else torch.int32))
               for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SWEEP)), ids=SWEEP_IDS)
def test_operands_between_guard_bands(device, strict, i):
    """Every operand a view between NaN guard bands, reaching the kernel as that view (the ops' ``.contiguous()`` and
    dtype conversions return it: same ``data_ptr()``): finite, within the bound, bitwise the unguarded result; guards
    and inputs unchanged."""
    f, m, n, k, fl = SWEEP[i]
    c = _case(f, m, n, k, **fl)
    plain = _run(c, _dev_args(c, device))
    guards, args = [], []
    for j, (t, role) in enumerate(zip(c.args, c.roles)):
        if not isinstance(t, torch.Tensor):
            args.append(t)
            continue
        assert role is not None and t.dtype == _kernel_dtype(c, role)
        g = Guarded(device, j, t)
        assert g.view.to(_kernel_dtype(c, role)).contiguous().data_ptr() == g.view.data_ptr()
        assert g.view.data_ptr() % 16 == 0
        guards.append(g)
        args.append(g.view)
    out = _run(c, args)
    torch.cuda.synchronize()
    for j, g in enumerate(guards):
        assert g.guards_intact(), f"guard of operand {j} changed"
        assert g.unchanged(), f"operand {j} changed"
    _check(c, out, "guarded")
    assert _same(out, plain)


NAN_WORD = 0x7FC07FC0  # NaN as fp32 and as either bf16 half


def _out_bytes(c):
    esz = 4 if c.out == 1 else 2
    n = c.ref.numel() * (2 if c.out == 2 else 1) * esz
    return [n] + ([c.M * (c.N // 64) * 2 * 4] if c.stats else [])


@pytest.mark.gpu
def test_every_output_element_is_written(device, strict):
    """Best effort (module docstring): a NaN-filled block of each output's exact byte size is freed right before the
    call; where the op's output is that block, every element of it must be finite afterwards.  A case whose output
    landed elsewhere is reported, and at most one may."""
    missed = []
    for i, (f, m, n, k, fl) in enumerate(SWEEP):
        c = _case(f, m, n, k, **fl)
        args = _dev_args(c, device)
        torch.cuda.synchronize()
        blocks = [torch.full((nb // 4,), NAN_WORD, dtype=torch.int32, device=device) for nb in _out_bytes(c)]
        assert all(bool(torch.isnan(b.view(F32)).all()) and bool(torch.isnan(b.view(BF)).all()) for b in blocks)
        ptrs = {b.data_ptr() for b in blocks}
        torch.cuda.synchronize()
        del blocks
        out = _run(c, args)
        outs = out if isinstance(out, tuple) else (out,)
        torch.cuda.synchronize()
        reused = all(o.data_ptr() in ptrs for o in outs) and len({o.data_ptr() for o in outs}) == len(outs)
        finite = all(bool(torch.isfinite(o.float()).all()) for o in outs)
        print(f"MEASURED gemm {c.form} written {c.name} block reused {reused} finite {finite}")
        assert finite, SWEEP_IDS[i]
        if not reused:
            missed.append(SWEEP_IDS[i])
    print(f"MEASURED gemm written checks not made: {len(missed)} of {len(SWEEP)} {missed}")
    assert len(missed) <= 1, missed


# K = 64 in bf16 (one K-tile: the second stage is never filled) | N = 64 (three quarters of the feature rows are
# clamped copies) | M = 1 | the staged epilogue with statistics at the base shape | both patch modes
STALE = [(f, m, n, k, fl) for key in ("fc1-bf16", "fc2-bf16") for f, fl in [TOKEN_FORMS[key]] for m, n, k in [(257, 320, 64)]] + \
    [(f, m, n, k, fl) for f, fl in TOKEN_FORMS.values() for m, n, k in [(257, 64, 192), (1, 320, 192)]] + \
    [(f, m, n, k, fl) for key in ("fc2-bf16", "fc2-x3") for f, fl in [TOKEN_FORMS[key]] for m, n, k in [BASE]] + \
    [p for p in PATCH_CASES if p[4]["grid"] == (3, 5, 7) and p[2] in (320, 256) and p[3] == 192]
STALE_IDS = [SWEEP_IDS[SWEEP.index(s)] for s in STALE]


@pytest.mark.gpu
@pytest.mark.xdist_group(name="stale_lds")
@pytest.mark.parametrize("i", range(len(STALE)), ids=STALE_IDS)
def test_stale_lds(device, strict, i):
    """The kernel launched right after ``lds_poison()`` (every operand already in the kernel's dtype, ``pre`` given:
    the op launches nothing else) gives the bits of the run before it."""
    f, m, n, k, fl = STALE[i]
    c = _case(f, m, n, k, **fl)
    args = _dev_args(c, device)
    first = _run(c, args)
    torch.cuda.synchronize()
    ops.lds_poison()
    assert float(ops.lds_probe()) == 1.0
    ops.lds_poison()
    out = _run(c, args)
    torch.cuda.synchronize()
    _check(c, out, "stale-lds")
    assert _same(out, first)


@pytest.mark.gpu
def test_worst_ratios_are_reported(device):
    """Prints the worst err / bound per form of this process's checks (the module docstring's table)."""
    for form, worst in sorted(_WORST.items()):
        print(f"MEASURED gemm worst err/bound {form} {worst:.3f}")
    assert all(w <= 1.0 for w in _WORST.values())
