"""The LayerNorm kernel family (csrc/spectral/layernorm.hip) per element: every instance, at the smallest width that
reaches it, at its partial-chunk edge and at its full edge, on rows that stress the statistics.

``torch.ops.amd_dft.ln_info(op, C, bf16)`` names the kernel a call takes (``ln_bf16<4>``, ``ln_stats_768``,
``ln_f32_split<2>`` ...: kernel<16-byte chunks per lane>); one table of cases (``CASES``) drives the CPU tier, the
mutation tier and the GPU tier, and a CPU test proves it reaches every name.

Reference: fp64 torch on the exact stored inputs.  ``x' = x + pre`` (or ``x + residual``) is never rounded before
the statistics, the variance is biased, eps = 1e-6.

Comparison: per element against a worst-case model of the kernels' fp32 arithmetic, not a whole-tensor norm.  With
u = 2^-24, S = (elements a lane sums) + 8 (six shuffle levels, the divide, one spare) and A = max_j |x'_j| of the row:

    mean     |dmean| <= delta = S u A
    rstd     |drstd| / rstd <= (S + 4) u + delta^2 rstd^2   (+ u A rstd with a fused addend, see rstd_rel_bound)
    y_i      |g_i| rstd (delta + 4 u |x'_i - mean|) + ((S + 6) u + delta^2 rstd^2) |g_i xhat_i| + 2 u |b_i|
             + one RNE rounding for a bf16 output, + the rounding of lo for hi + lo of a split output

The rounding terms are exact half ulps, not a multiple of |y_i|: bf16 keeps 8 significand bits, so one RNE rounding
moves y by up to h(y) = 2^(floor(log2 |y|) - 8), which lies between 2^-9 |y| and 2^-8 |y|; lo = bf16(y - hi) rounds
a value of at most h(y), so hi + lo misses y by up to 2^-8 h(y) (2^-17 |y| .. 2^-16 |y|).  A flat 2^-9 |y| (2^-17 |y|)
is not a bound of a rounding: the fp64 reference itself, rounded once, exceeds it 1.8-fold in the lower half of
every binade (0.2744 -> 0.2734 is off by 2^-10 = 2^-8.1 |y|).  The binade is taken at |y| + the fp32 bound, since
the kernel rounds its own fp32 value.

The constants come from the kernels' summation depth, none is measured.  The CPU ops and the ATen fallback sum
differently and are held to the same model with S = C (the only looser check).  ``MEASURED`` lines print the worst
|out - ref| / bound of every case; the MI355X values are recorded beside ``WORST_ON_MI355X``.

The mutation tier (CPU) feeds the same comparison the fp64 reference with one defect and proves it is rejected for
every instance the defect applies to (``MUTATIONS`` / ``NOT_SEEN``).
"""
import math
import re

import pytest
import torch

from tensorrt_dft_plugins_amd.ops import spectral as S
from test_afno_w import merge_inputs

ops = torch.ops.amd_dft
BF16, F32 = torch.bfloat16, torch.float32
EPS = 1e-6
U = 2.0 ** -24

# widths: the smallest that reach each instance, its partial-chunk edge and its full edge -> chunks per lane
W_BF16 = {8: 1, 72: 1, 504: 1, 512: 1, 520: 2, 768: 2, 1024: 2, 1032: 4, 1544: 4, 2048: 4}
W_F32 = {4: 1, 252: 1, 256: 1, 260: 2, 512: 2, 516: 3, 768: 3, 772: 4, 1024: 4, 1028: 8, 2044: 8, 2048: 8}
W_SPLIT = {32: 1, 224: 1, 256: 1, 288: 2, 512: 2, 544: 3, 768: 3, 800: 4, 1024: 4, 1056: 8, 2048: 8}


def _cases():
    """(op, dtype, C, add, rows): add = a residual (layer_norm, bf16 only) or a per-channel pre (ln_stats,
    layer_norm_split).  9 rows = two workgroups of 4 waves plus one wave (the 768 statistics kernel: one group of 8
    rows plus a lone first-of-pair row); 1 row = a lone wave."""
    out = []
    for C in W_BF16:
        for rows in (9, 1) + ((2, 7, 8) if C == 768 else ()):
            for add in (False, True):
                if rows in (9, 1):
                    out.append(("layer_norm", BF16, C, add, rows))
                out.append(("ln_stats", BF16, C, add, rows))
    for C in W_F32:
        for rows in (9, 1):
            out.append(("layer_norm", F32, C, False, rows))
            out += [("ln_stats", F32, C, add, rows) for add in (False, True)]
    for C in W_SPLIT:
        for rows in (9, 1):
            out += [("layer_norm_split", F32, C, add, rows) for add in (False, True)]
    return out


CASES = _cases()


def case_id(case):
    op, dt, C, add, rows = case
    return f"{op}-{'bf16' if dt == BF16 else 'f32'}-C{C}-{'add' if add else 'plain'}-r{rows}"


def info(case):
    op, dt, C, add, _ = case
    return ops.ln_info("layer_norm_res" if op == "layer_norm" and add else op, C, dt == BF16)


def table_info(case):
    """The name the width tables above promise (no op library needed: parametrisation happens at collection);
    test_ln_info_routes and test_cases_reach_every_kernel hold ln_info to it"""
    op, dt, C, add, _ = case
    if op == "layer_norm_split":
        return "ln_split_lds<3>" if C == 768 else f"ln_f32_split<{W_SPLIT[C]}>"
    if dt == F32:
        return f"{'ln_f32' if op == 'layer_norm' else 'ln_f32_stats'}<{W_F32[C]}>"
    if op == "ln_stats":
        return "ln_stats_768" if C == 768 else f"ln_stats<{W_BF16[C]}>"
    return f"{'ln_bf16_res' if add else 'ln_bf16'}<{W_BF16[C]}>"


def geometry(inst):
    """(elements per 16-byte chunk, chunks per lane) of an ln_info name: a lane sums their product"""
    m = re.fullmatch(r"(ln_[a-z0-9_]+?)(?:<(\d+)>)?", inst)
    assert m, inst
    name = m.group(1)
    if name == "ln_stats_768":
        return 8, 3  # 24 elements per lane: three chunks of the two-row span
    assert name in ("ln_bf16", "ln_bf16_res", "ln_stats", "ln_f32", "ln_f32_stats", "ln_f32_split", "ln_split_lds"), inst
    return (8 if name in ("ln_bf16", "ln_bf16_res", "ln_stats") else 4), int(m.group(2))


FIXED_768 = ("ln_stats_768", "ln_split_lds<3>")  # kernels of one width: every lane full, no mask, no clamp


def partial(case):
    """The width leaves the last 64-chunk step of the case's kernel partly filled (masks and clamped index at work)"""
    inst = table_info(case)
    return inst not in FIXED_768 and (case[2] // geometry(inst)[0]) % 64 != 0


def depth(inst):
    e, n = geometry(inst)
    return e * n + 8


# ------------------------------------------------------------------ inputs
_INPUTS = {}
SEED = 3 << 20  # chosen so that every split case stays under 1 % rounding ties on the CPU op (test_instance_cpu checks)


def make_inputs(case):
    """Five row kinds, cycled: (a) mean 0 std 1, (b) mean 3 std 2, (c) mean -100 std 1, (d) constant, (e) std 30 with
    one 200x outlier in the last channel.  gamma 1 + 0.3 randn with one exact 0 and one negative entry, beta
    0.1 randn, pre 0.2 randn; a residual is 0.5 randn (constant on the constant rows, so x' stays constant there).
    Everything is stored in the dtype the kernel reads, and the reference starts from those stored values."""
    if case in _INPUTS:
        return _INPUTS[case]
    op, dt, C, add, rows = case
    gen = torch.Generator().manual_seed(SEED + C * 64 + rows)
    x = torch.empty(rows, C)
    res = 0.5 * torch.randn(rows, C, generator=gen)
    for r in range(rows):
        z = torch.randn(C, generator=gen)
        kind = "abcde"[r % 5]
        if kind == "a":
            x[r] = z
        elif kind == "b":
            x[r] = 3 + 2 * z
        elif kind == "c":
            x[r] = -100 + z
        elif kind == "d":
            x[r] = 2.5
            res[r] = 0.75
        else:
            x[r] = 30 * z
            x[r, C - 1] = 200 * 30
    gam = 1 + 0.3 * torch.randn(C, generator=gen)
    gam[1] = 0.0
    gam[C - 2] = -0.7
    bet = 0.1 * torch.randn(C, generator=gen)
    pre = 0.2 * torch.randn(C, generator=gen)
    x = x.to(dt)
    if op == "layer_norm" and dt == BF16:
        gam, bet = gam.to(BF16), bet.to(BF16)
    extra = None
    if add:
        extra = res.to(BF16) if op == "layer_norm" else pre
    t = dict(x=x, g=gam, b=bet, add=extra)
    _INPUTS[case] = t
    return t


# ------------------------------------------------------------------ fp64 reference (and its mutations)
MUTATIONS = {
    # name: (ops it applies to, needs `add`, needs more than one row)
    "padded_divisor": (("layer_norm", "ln_stats", "layer_norm_split"), None, False),   # sum / (lanes * elements)
    "drop_last_chunk": (("layer_norm", "ln_stats", "layer_norm_split"), None, False),  # last partial 16-byte chunk
    "gamma_chunk0": (("layer_norm", "layer_norm_split"), None, False),                 # gamma of chunk 0 on the last
    "beta_chunk0": (("layer_norm", "layer_norm_split"), None, False),
    "no_eps": (("layer_norm", "ln_stats", "layer_norm_split"), None, False),
    "unbiased": (("layer_norm", "ln_stats", "layer_norm_split"), None, False),
    "pre_twice": (("ln_stats", "layer_norm_split"), True, False),
    "pre_dropped": (("ln_stats", "layer_norm_split"), True, False),
    "row_shift": (("layer_norm", "ln_stats", "layer_norm_split"), None, True),        # stats of row r - 1
    "res_xout_truncated": (("layer_norm",), True, False),   # x_out packed by truncation instead of one RNE rounding
    "res_y_from_rounded": (("layer_norm",), True, False),   # y normalised from the rounded x_out
    "lo_from_unrounded_hi": (("layer_norm_split",), None, False),  # lo = bf16(y - y) = 0
    "hi_lo_swapped": (("layer_norm_split",), None, False),
    "group_shift": (("layer_norm_split",), None, False),    # k32 interleave off by one 32-column group
}

# (mutation, instance) pairs the comparison cannot see, each with its reason.  Everything else must be rejected.
NOT_SEEN = {
    # fixed-width kernels: 768 channels fill every lane, there is no padded lane and no partial chunk
    ("padded_divisor", "ln_stats_768"): "768 = lanes x elements: the padded divisor is cols",
    ("padded_divisor", "ln_split_lds<3>"): "768 = lanes x elements: the padded divisor is cols",
    ("drop_last_chunk", "ln_stats_768"): "no partial chunk at 768",
    ("drop_last_chunk", "ln_split_lds<3>"): "no partial chunk at 768",
}
# Width condition of `unbiased` (rstd off by 1 / (2 C) relative): a bf16 output rounds at 2^-9, so above C = 512 the
# defect is below one output rounding and only a fraction of the elements exceed the bound.  It is therefore pinned
# through the fp32 ln_stats output at EVERY width (test_unbiased_variance_rejected_through_stats) and through bf16
# layer_norm at C = 8 and C = 72; the tier below still demands a rejecting case for the wider bf16 instances.
# Width condition of `padded_divisor` / `drop_last_chunk`: only a width whose chunk count is no multiple of 64 has a
# padded lane or a partial chunk; at the full edges (512, 1024, 2048 ...) the mutation is the identity.


def _truncate_bf16(v):
    return (v.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


def ln_ref(case, mut=None):
    """fp64 LayerNorm of the case's stored inputs -> dict(xp, mean, rstd, A, xhat, y, g, b); ``mut``: one defect"""
    op, dt, C, add, rows = case
    t = make_inputs(case)
    e, nch = geometry(info(case))
    x, a = t["x"].double(), (0.0 if t["add"] is None else t["add"].double())
    if mut == "pre_twice":
        a = 2 * a
    if mut == "pre_dropped":
        a = 0.0
    xp = x + a
    if mut == "res_y_from_rounded":
        xp = (t["x"].float() + t["add"].float()).to(BF16).double()
    xs, n = xp, float(C)
    if mut == "padded_divisor":
        n = float(64 * e * nch) if info(case) != "ln_stats_768" else 768.0
    if mut == "drop_last_chunk" and partial(case):
        xs = xp[:, :C - e]
    mean = xs.sum(-1) / n
    var = (xs - mean[:, None]).pow(2).sum(-1) / n
    if mut == "unbiased":
        var = var * C / (C - 1)
    rstd = torch.rsqrt(var + (0.0 if mut == "no_eps" else EPS))
    if mut == "row_shift":
        mean, rstd = mean.roll(1), rstd.roll(1)
    g, b = t["g"].double().clone(), t["b"].double().clone()
    if mut == "gamma_chunk0":
        g[C - e:] = g[:e]
    if mut == "beta_chunk0":
        b[C - e:] = b[:e]
    xhat = (xp - mean[:, None]) * rstd[:, None]
    return dict(xp=xp, mean=mean, rstd=rstd, A=xp.abs().amax(-1), xhat=xhat, y=xhat * g + b, g=g, b=b)


_REF = {}


def reference(case):
    if case not in _REF:
        _REF[case] = ln_ref(case)
    return _REF[case]


def interleave(hi, lo):
    """[rows, C] hi, lo -> [rows, 2C] k32-interleaved: every 32 columns stored as [hi(32) | lo(32)]"""
    r, C = hi.shape
    return torch.stack([hi.reshape(r, C // 32, 32), lo.reshape(r, C // 32, 32)], 2).reshape(r, 2 * C)


def emit(case, R, mut=None):
    """What a kernel computing R exactly would store: the op's outputs, rounded once to their formats"""
    op, dt, C, add, rows = case
    t = make_inputs(case)
    if op == "ln_stats":
        return (torch.stack([R["mean"], R["rstd"]], 1).float(),)
    y32 = R["y"].float()
    if op == "layer_norm":
        xo = t["x"]
        if add:
            s = t["x"].float() + t["add"].float()
            xo = _truncate_bf16(s) if mut == "res_xout_truncated" else s.to(BF16)
        return y32.to(dt), xo
    hi = y32.to(BF16)
    lo = (y32 - (y32 if mut == "lo_from_unrounded_hi" else hi.float())).to(BF16)
    if mut == "hi_lo_swapped":
        hi, lo = lo, hi
    ys = interleave(hi, lo)
    if mut == "group_shift":
        ys = ys.roll(64, 1)
    return (ys,)


# ------------------------------------------------------------------ comparison
def _ratio(diff, bound):
    """worst diff / bound; a difference where the bound is zero, or anything not finite, is infinite"""
    if not bool(torch.isfinite(diff).all()):
        return math.inf
    zero = bound <= 0
    if bool((diff[zero] > 0).any()):
        return math.inf
    return float((diff / torch.where(zero, torch.ones_like(bound), bound)).max())


def rstd_rel_bound(R, depth_, add):
    """(S + 4) u + delta^2 rstd^2, plus u A rstd where an addend is fused: x_i + pre_i is rounded to fp32 before the
    statistics (|e_i| <= u A), and unlike an error of the mean these do not cancel in the variance:
    |dvar| <= 2 u A mean|d_i| <= 2 u A / rstd, so |drstd| / rstd <= u A rstd.  Without an addend x' is the stored x."""
    delta = depth_ * U * R["A"]
    return (depth_ + 4) * U + (delta * R["rstd"]).pow(2) + (U * R["A"] * R["rstd"] if add else 0.0)


def stats_ratio(st, R, depth_, add):
    st = st.detach().double().cpu()
    if st.shape != (R["mean"].numel(), 2):
        return math.inf
    rm = _ratio((st[:, 0] - R["mean"]).abs(), depth_ * U * R["A"])
    rr = _ratio((st[:, 1] / R["rstd"] - 1).abs(), rstd_rel_bound(R, depth_, add))
    return max(rm, rr)


def half_ulp_bf16(v):
    """Half a bf16 ulp at magnitude v (8 significand bits): 2^(floor(log2 v) - 8), the most one RNE rounding moves v"""
    return torch.exp2(torch.floor(torch.log2(v.clamp_min(1e-300))) - 8)


def y_bound(R, depth_, fmt, add):
    """fmt: "f32", "bf16" (one RNE rounding of the fp32 result) or "split" (hi + lo: the rounding of lo, which is at
    most half an ulp of hi's own rounding error)"""
    delta, rstd = (depth_ * U * R["A"])[:, None], R["rstd"][:, None]
    f32 = R["g"].abs() * rstd * (delta + 4 * U * (R["xp"] - R["mean"][:, None]).abs()) \
        + (2 * U + rstd_rel_bound(R, depth_, add)[:, None]) * (R["g"] * R["xhat"]).abs() + 2 * U * R["b"].abs()
    if fmt == "f32":
        return f32
    return f32 + half_ulp_bf16(R["y"].abs() + f32) * (1.0 if fmt == "bf16" else 2.0 ** -8)


def split_structure(ys, C):
    """The pair row per 32-column group [hi(32) | lo(32)]: (hi, lo, ties); None where a group is no split pair:
    |lo| <= 2^-8 |hi| and bf16(hi + lo) == hi except where lo is exactly half the gap to the next bf16 (a tie of
    the first rounding, which may resolve either way)."""
    r = ys.shape[0]
    grp = ys.detach().cpu().reshape(r, C // 32, 2, 32)
    hi, lo = grp[:, :, 0].float(), grp[:, :, 1].float()
    if bool((lo.abs() > 2.0 ** -8 * hi.abs()).any()):
        return None
    back = (hi + lo).to(BF16).float()
    off = back != hi
    two = hi + 2 * lo
    tie = off & (two.to(BF16).float() == two) & (lo != 0)
    if bool((off & ~tie).any()):
        return None
    return hi.reshape(r, C), lo.reshape(r, C), int(tie.sum())


def verdict(case, outs, depth_):
    """Worst |out - ref| / bound of an op's outputs for the case (inf: a structural check failed)"""
    op, dt, C, add, rows = case
    R, t = reference(case), make_inputs(case)
    if op == "ln_stats":
        return stats_ratio(outs[0], R, depth_, add)
    if op == "layer_norm":
        y, xo = outs
        if y.dtype != dt or y.shape != (rows, C):
            return math.inf
        want = (t["x"].float() + t["add"].float()).to(BF16) if add else t["x"]
        if xo.shape != want.shape or not torch.equal(xo.detach().cpu(), want):  # x_out: one RNE rounding of the sum
            return math.inf
        return _ratio((y.detach().double().cpu() - R["y"]).abs(), y_bound(R, depth_, "bf16" if dt == BF16 else "f32", add))
    ys = outs[0]
    if ys.dtype != BF16 or ys.shape != (rows, 2 * C):
        return math.inf
    parts = split_structure(ys, C)
    if parts is None:
        return math.inf
    hi, lo, ties = parts
    if ties >= 0.01 * hi.numel():
        return math.inf
    return _ratio((hi.double() + lo.double() - R["y"]).abs(), y_bound(R, depth_, "split", add))


def run(case, device):
    op, dt, C, add, rows = case
    t = make_inputs(case)
    d = lambda v: None if v is None else v.to(device)  # noqa: E731
    if op == "ln_stats":
        return (ops.ln_stats(d(t["x"]), d(t["add"]), EPS),)
    if op == "layer_norm":
        return tuple(ops.layer_norm(d(t["x"]), d(t["g"]), d(t["b"]), EPS, d(t["add"])))
    return (ops.layer_norm_split(d(t["x"]), d(t["g"]), d(t["b"]), EPS, d(t["add"])),)


# Worst |out - ref| / bound per instance over the GPU tier below, as printed by its MEASURED lines on an MI355X
# (nothing here is a tolerance: the bound is the model of the module docstring and the limit is 1).
# The bf16 outputs sit just under 1 by construction: one RNE rounding uses its half ulp almost fully on some element,
# the fp32 part of the bound is the margin.
WORST_ON_MI355X = {
    "ln_bf16<1>": 0.997, "ln_bf16<2>": 0.998, "ln_bf16<4>": 0.997,              # C 504, 1024 (1 row), 1544
    "ln_bf16_res<1>": 0.997, "ln_bf16_res<2>": 0.998, "ln_bf16_res<4>": 0.997,  # C 504, 1024 (1 row), 1032 (1 row)
    "ln_stats<1>": 0.151, "ln_stats<2>": 0.060, "ln_stats<4>": 0.070, "ln_stats_768": 0.083,  # C 8 + pre, 1024, 2048, 8 rows
    "ln_f32<1>": 0.091, "ln_f32<2>": 0.105, "ln_f32<3>": 0.051, "ln_f32<4>": 0.056, "ln_f32<8>": 0.128,  # C 252, 260, 768, 1024, 2044
    "ln_f32_stats<1>": 0.119, "ln_f32_stats<2>": 0.105, "ln_f32_stats<3>": 0.073, "ln_f32_stats<4>": 0.060,
    "ln_f32_stats<8>": 0.068,                                                   # C 4 + pre, 260, 768, 1024, 1028
    "ln_f32_split<1>": 0.420, "ln_f32_split<2>": 0.407, "ln_f32_split<3>": 0.415, "ln_f32_split<4>": 0.441,
    "ln_f32_split<8>": 0.357, "ln_split_lds<3>": 0.380,                         # C 224, 288, 544, 1024, 1056, 768
}


def test_recorded_worst_names_every_kernel():
    assert set(WORST_ON_MI355X) == ALL_KERNELS and max(WORST_ON_MI355X.values()) <= 1


# ------------------------------------------------------------------ CPU tier: routes
def test_ln_info_routes():
    inf = ops.ln_info
    for C, n in W_BF16.items():
        assert inf("layer_norm", C, True) == f"ln_bf16<{n}>"
        assert inf("layer_norm_res", C, True) == f"ln_bf16_res<{n}>"
        assert inf("ln_stats", C, True) == ("ln_stats_768" if C == 768 else f"ln_stats<{n}>")
    for C, n in W_F32.items():
        assert inf("layer_norm", C, False) == f"ln_f32<{n}>"
        assert inf("ln_stats", C, False) == f"ln_f32_stats<{n}>"
        assert inf("layer_norm_res", C, False) == "fallback"  # a residual needs bf16
    for C, n in W_SPLIT.items():
        assert inf("layer_norm_split", C, False) == ("ln_split_lds<3>" if C == 768 else f"ln_f32_split<{n}>")
    for op in ("layer_norm", "layer_norm_res", "ln_stats"):
        assert inf(op, 12, True) == "fallback" and inf(op, 2056, True) == "fallback"
    for op in ("layer_norm", "ln_stats"):
        assert inf(op, 6, False) == "fallback" and inf(op, 2056, False) == "fallback"
    assert inf("layer_norm_split", 48, False) == "error" and inf("layer_norm_split", 2080, False) == "error"
    assert inf("layer_norm_split", 768, True) == "error"  # split rows are fp32
    with pytest.raises(RuntimeError):
        inf("layer_norm_fused", 768, True)
    with pytest.raises(RuntimeError):
        inf("layer_norm", 0, True)


# every kernel of layernorm.hip that ships (the two MI_DFT_LN_SPLIT=dup instances exist in tuning builds only)
ALL_KERNELS = {f"{k}<{n}>" for k in ("ln_bf16", "ln_bf16_res", "ln_stats") for n in (1, 2, 4)} | {"ln_stats_768"} | \
    {f"{k}<{n}>" for k in ("ln_f32", "ln_f32_stats", "ln_f32_split") for n in (1, 2, 3, 4, 8)} | {"ln_split_lds<3>"}


def test_cases_reach_every_kernel():
    """Every name ln_info can return is run by a 9-row case, with and without `add` where the op takes one, at a
    width with a partial chunk and at a full one where the kernel takes both"""
    seen = {}
    for case in CASES:
        assert info(case) == table_info(case), case_id(case)
        seen.setdefault(info(case), []).append(case)
    assert set(seen) == ALL_KERNELS, set(seen) ^ ALL_KERNELS
    for inst, cases in seen.items():
        e, n = geometry(inst)
        assert any(c[4] == 9 for c in cases) and any(c[4] == 1 for c in cases), inst
        if not inst.startswith(("ln_bf16", "ln_f32<")):  # the ops with an optional pre
            assert {c[3] for c in cases} == {False, True}, inst
        if inst not in FIXED_768:
            assert any(partial(c) for c in cases), inst  # a partial chunk: masks, clamped index
            if inst != "ln_f32_split<3>":  # its full edge, 768, belongs to ln_split_lds<3>
                assert any(c[2] == 64 * e * n for c in cases), inst  # the full edge


def test_row_kinds():
    """What the row kinds promise, on the stored values"""
    for case in (("layer_norm", BF16, 72, False, 9), ("layer_norm", F32, 2044, False, 9), ("ln_stats", BF16, 768, True, 9)):
        R = reference(case)
        std = 1 / R["rstd"]
        assert (R["mean"][2].abs() / std[2]).item() > 50  # (c): |mean| / std >> 1
        assert R["mean"][1].item() > 2 and 1.5 < std[1].item() < 2.5
        assert R["xp"][4].abs().argmax().item() == case[2] - 1  # (e): the outlier sits in the last valid channel
        t = make_inputs(case)
        assert bool((t["g"] == 0).any()) and bool((t["g"] < 0).any())
    R = reference(("layer_norm", BF16, 72, True, 9))
    assert R["rstd"][3].item() == pytest.approx(1000.0, rel=1e-9) and R["rstd"][8].item() == pytest.approx(1000.0, rel=1e-9)


# ------------------------------------------------------------------ CPU tier: the CPU ops within the bounds
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_instance_cpu(case):
    """The CPU ops at the same inputs and bounds, with S = C (ATen sums differently); the split inputs stay under
    1 % rounding ties"""
    op, dt, C, add, rows = case
    outs = run(case, "cpu")
    r = verdict(case, outs, C)
    assert r <= 1, f"{case_id(case)}: {r:.3f}"
    if op == "layer_norm_split":
        assert split_structure(outs[0], C)[2] < 0.01 * rows * C


@pytest.mark.parametrize("rows", [True, False])
def test_split_bf16_cpu(rows):
    """The CPU split against a reference written here: hi = bf16(x), lo = bf16(x - hi), per 32-column group"""
    x = _split_input((5, 2080) if rows else (2048 + 8,))
    y = ops.split_bf16(x, rows)
    hi = x.to(BF16)
    lo = (x - hi.float()).to(BF16)
    if not rows:
        assert torch.equal(y, torch.stack([hi, lo]))
        return
    grp = y.reshape(5, 65, 2, 32)
    assert torch.equal(grp[:, :, 0], hi.reshape(5, 65, 32)) and torch.equal(grp[:, :, 1], lo.reshape(5, 65, 32))


def test_wrong_sizes_cpu():
    x, g, b = torch.randn(3, 72), torch.ones(72), torch.zeros(72)
    for n in (64, 80):
        with pytest.raises(RuntimeError):
            ops.layer_norm(x, torch.ones(n), b, EPS, None)
        with pytest.raises(RuntimeError):
            ops.layer_norm(x, g, torch.zeros(n), EPS, None)


# ------------------------------------------------------------------ CPU tier: mutations
def _applies(mut, case):
    op, dt, C, add, rows = case
    on, need_add, need_rows = MUTATIONS[mut]
    if op not in on or (need_add and not add) or (need_rows and rows < 2):
        return False
    return not (mut.startswith("res_") and dt != BF16)


def rejects(case, mut):
    return verdict(case, emit(case, ln_ref(case, mut), mut), depth(info(case))) > 1


_PAIRS = sorted({(m, table_info(c)) for m in MUTATIONS for c in CASES if _applies(m, c)})


@pytest.mark.parametrize("mut,inst", _PAIRS)
def test_bound_rejects_mutation(mut, inst):
    """The comparison accepts the rounded fp64 reference at the instance's own S and rejects the reference with one
    defect, for at least one width and row count of the GPU table, for every instance the defect applies to"""
    cases = [c for c in CASES if info(c) == inst and _applies(mut, c)]
    assert cases
    for c in cases:
        assert verdict(c, emit(c, reference(c)), depth(inst)) <= 1, case_id(c)
    hit = [case_id(c) for c in cases if rejects(c, mut)]
    print(f"layernorm mutation {mut} {inst}: rejected at {len(hit)} of {len(cases)} cases")
    if (mut, inst) in NOT_SEEN:
        assert not hit, f"{mut} {inst} is seen after all ({hit}): drop it from NOT_SEEN"
        return
    assert hit, f"no case of {inst} rejects {mut}"


def test_not_seen_pairs_exist():
    assert set(NOT_SEEN) <= set(_PAIRS)


def test_unbiased_variance_rejected_through_stats():
    """The width condition of `unbiased`: rejected through the fp32 statistics at every width of both dtypes, with
    and without pre, and through the bf16 layer_norm output at C = 8 and C = 72"""
    for c in CASES:
        op, dt, C, add, rows = c
        if op == "ln_stats" or (op == "layer_norm" and dt == BF16 and C in (8, 72)):
            assert rejects(c, "unbiased"), case_id(c)


def test_partial_width_mutations_rejected_at_every_partial_width():
    """Stronger than one case per instance: a padded divisor and a dropped last chunk are rejected at EVERY width with
    a partial chunk, on 9 rows, in every op"""
    for c in CASES:
        op, dt, C, add, rows = c
        if rows == 9 and partial(c):
            assert rejects(c, "drop_last_chunk") and rejects(c, "padded_divisor"), case_id(c)


# ------------------------------------------------------------------ GPU tier
def _embedded(v, device, offset):
    """v as a contiguous view `offset` elements into a larger NaN-filled device buffer (>= 64 elements either side)"""
    buf = torch.full((v.numel() + 256,), math.nan, dtype=v.dtype, device=device)
    view = buf[offset:offset + v.numel()].view(v.shape)
    view.copy_(v)
    return view


def _run_embedded(case, device, offsets):
    """run() with each named input embedded at its offset (elements); all others plain device tensors"""
    op, dt, C, add, rows = case
    t = make_inputs(case)
    e = {k: (None if v is None else _embedded(v, device, offsets[k]) if k in offsets else v.to(device)) for k, v in t.items()}
    if op == "ln_stats":
        return (ops.ln_stats(e["x"], e["add"], EPS),)
    if op == "layer_norm":
        return tuple(ops.layer_norm(e["x"], e["g"], e["b"], EPS, e["add"]))
    return (ops.layer_norm_split(e["x"], e["g"], e["b"], EPS, e["add"]),)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_instance_gpu(device, case):
    """Every case on its kernel (no fallback recorded): the per-element bound at the instance's own S, x_out bit-equal
    to one rounding of the fp32 sum, the split pair structure per 32-column group"""
    inst = info(case)
    S.fallback_reset()
    outs = run(case, device)
    assert S.fallback_counts() == {}
    r = verdict(case, outs, depth(inst))
    print(f"MEASURED layernorm {inst} {case_id(case)} worst |out - ref| / bound {r:.3f}")
    assert r <= 1, f"{case_id(case)} on {inst}: {r:.3f}"


def _split_input(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-20, 20, shape, generator=g).float())
    x.reshape(-1)[:4] = torch.tensor([0.0, -0.0, 1.0, 1.00390625])  # exact zeros, an exact bf16, an exact tie
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("shape,rows", [((9, 32), True), ((5, 2080), True), ((3, 768), True),
                                        ((8,), False), ((2048 + 8,), False), ((3 * 2048,), False)])
def test_split_bf16_gpu(device, shape, rows):
    """split_bf16 is exact: bit equality with the CPU op (itself pinned by test_split_bf16_cpu).  Planes: a single
    thread, a one-thread tail workgroup, full workgroups."""
    x = _split_input(shape)
    y = ops.split_bf16(x.to(device), rows)
    assert torch.equal(y.cpu(), ops.split_bf16(x, rows))
    assert torch.equal(S.split_bf16(x.to(device), rows).cpu(), y.cpu())


def _partial_case(inst):
    e, n = geometry(inst)
    want_add = not inst.startswith(("ln_bf16<", "ln_f32<"))
    for c in CASES:
        if table_info(c) == inst and c[4] == 9 and c[3] == want_add and (partial(c) or inst in FIXED_768):
            return c
    raise AssertionError(inst)


@pytest.mark.gpu
@pytest.mark.parametrize("inst", sorted(ALL_KERNELS))
def test_poisoned_surroundings_gpu(device, inst):
    """Every input a 16-byte-aligned view 64 elements into a NaN-filled buffer, at one partial-chunk width per
    instance: bit-identical to the plain run and finite (a read past the row end, which the clamped chunk index
    prevents, would bring a NaN in)"""
    case = _partial_case(inst)
    plain = run(case, device)
    inside = _run_embedded(case, device, {k: 64 for k in ("x", "g", "b", "add")})
    for a, b in zip(plain, inside):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("layer_norm", BF16, 8, True, 9), ("layer_norm", F32, 4, False, 9),
                                  ("ln_stats", BF16, 8, True, 9), ("ln_stats", F32, 4, True, 9),
                                  ("layer_norm_split", F32, 32, True, 9)], ids=case_id)
def test_misaligned_views_gpu(device, case):
    """Each input in turn a contiguous view ONE element into a larger buffer (not 16-byte aligned: the ops copy it), at
    the smallest partial-chunk width of each dtype: bit-identical to the aligned call"""
    op = case[0]
    plain = run(case, device)
    for name in ("x", "add") + (() if op == "ln_stats" else ("g", "b")):
        if make_inputs(case)[name] is None:
            continue
        off = _run_embedded(case, device, {name: 1})
        for a, b in zip(plain, off):
            assert torch.equal(a, b), name


@pytest.mark.gpu
def test_misaligned_split_and_merge_gpu(device):
    for shape, rows in (((9, 32), True), ((8,), False)):
        x = _split_input(shape)
        assert torch.equal(ops.split_bf16(_embedded(x, device, 1), rows), ops.split_bf16(x.to(device), rows))
    part, shift = merge_inputs(5, 3)
    plain = ops.ln_stats_merge(part.to(device), EPS, shift.to(device))
    assert torch.equal(ops.ln_stats_merge(_embedded(part, device, 1), EPS, shift.to(device)), plain)
    assert torch.equal(ops.ln_stats_merge(part.to(device), EPS, _embedded(shift, device, 1)), plain)
    assert torch.equal(ops.ln_stats_merge(_embedded(part, device, 1), EPS, None), ops.ln_stats_merge(part.to(device), EPS, None))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
def test_wrong_sizes_gpu(device, dt):
    """gamma / beta with C - 8 or C + 8 entries, pre with C - 4, a residual of another shape: RuntimeError on the host,
    on the bf16 and the fp32 route of layer_norm (the check sits before any conversion or launch)"""
    C = 72
    x = torch.randn(9, C).to(dt).to(device)
    g, b = torch.ones(C, device=device), torch.zeros(C, device=device)
    for n in (C - 8, C + 8):
        with pytest.raises(RuntimeError, match="must have C"):
            ops.layer_norm(x, torch.ones(n, device=device), b, EPS, None)
        with pytest.raises(RuntimeError, match="must have C"):
            ops.layer_norm(x, g, torch.zeros(n, device=device), EPS, None)
    with pytest.raises(RuntimeError, match="one entry per channel"):
        ops.ln_stats(x, torch.zeros(C - 4, device=device), EPS)
    with pytest.raises(RuntimeError, match="residual shape"):
        ops.layer_norm(x, g, b, EPS, x[:8])
    with pytest.raises(RuntimeError, match="residual shape"):
        ops.layer_norm(x, g, b, EPS, x[:1])
    if dt == F32:
        xs = torch.randn(9, 96, device=device)
        g96, b96 = torch.ones(96, device=device), torch.zeros(96, device=device)
        with pytest.raises(RuntimeError, match="must have C"):
            ops.layer_norm_split(xs, g96, b96, EPS, torch.zeros(92, device=device))
        for n in (88, 104):
            with pytest.raises(RuntimeError, match="must have C"):
                ops.layer_norm_split(xs, torch.ones(n, device=device), b96, EPS, None)
            with pytest.raises(RuntimeError, match="must have C"):
                ops.layer_norm_split(xs, g96, torch.zeros(n, device=device), EPS, None)
        for C2 in (48, 2080):
            with pytest.raises(RuntimeError):
                ops.layer_norm_split(torch.randn(2, C2, device=device), torch.ones(C2, device=device),
                                     torch.zeros(C2, device=device), EPS, None)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("layer_norm", BF16, 12, False, 9), ("layer_norm", BF16, 12, True, 9),
                                  ("ln_stats", BF16, 12, True, 9), ("layer_norm", BF16, 2056, False, 9),
                                  ("ln_stats", BF16, 2056, False, 9), ("layer_norm", F32, 2056, False, 9),
                                  ("ln_stats", F32, 2056, True, 9), ("layer_norm", F32, 6, False, 9),
                                  ("ln_stats", F32, 6, False, 9)], ids=case_id)
def test_fallback_widths_gpu(device, case):
    """Widths no kernel takes go to ATen: still within the CPU-tier bound (S = C), counted, and refused under strict"""
    op, dt, C, add, rows = case
    assert ops.ln_info("layer_norm_res" if op == "layer_norm" and add else op, C, dt == BF16) == "fallback"
    S.fallback_reset()
    outs = run(case, device)
    assert S.fallback_counts().get(op, 0) == 1, S.fallback_counts()
    S.fallback_reset()
    r = verdict_plain(case, outs)
    print(f"MEASURED layernorm fallback {case_id(case)} worst |out - ref| / bound {r:.3f}")
    assert r <= 1
    prev = ops.set_strict(True)
    try:
        with pytest.raises(RuntimeError, match="MI_DFT_STRICT"):
            run(case, device)
    finally:
        ops.set_strict(prev)


def verdict_plain(case, outs):
    """verdict() for a width outside the tables (the reference needs no instance geometry): S = C"""
    _REF[case] = _ref_no_geometry(case)
    return verdict(case, outs, case[2])


def _ref_no_geometry(case):
    t = make_inputs(case)
    xp = t["x"].double() + (0.0 if t["add"] is None else t["add"].double())
    var, mean = torch.var_mean(xp, dim=-1, correction=0)
    rstd = torch.rsqrt(var + EPS)
    g, b = t["g"].double(), t["b"].double()
    xhat = (xp - mean[:, None]) * rstd[:, None]
    return dict(xp=xp, mean=mean, rstd=rstd, A=xp.abs().amax(-1), xhat=xhat, y=xhat * g + b, g=g, b=b)


@pytest.mark.parametrize("case", [("layer_norm", BF16, 12, True, 9), ("ln_stats", F32, 2056, True, 9),
                                  ("layer_norm", F32, 6, False, 9)], ids=case_id)
def test_fallback_widths_cpu(case):
    assert verdict_plain(case, run(case, "cpu")) <= 1


@pytest.mark.gpu
def test_none_optionals_gpu(device):
    """None for every optional tensor, through torch.ops and through the package's Python wrapper (layer_norm is the
    one LayerNorm op with one): the kernel runs, no fallback is recorded, results equal the positional call"""
    c16, c32, csp = ("layer_norm", BF16, 72, False, 9), ("ln_stats", F32, 260, False, 9), ("layer_norm_split", F32, 288, False, 9)
    S.fallback_reset()
    t = {k: v.to(device) for k, v in make_inputs(c16).items() if v is not None}
    y, xo = ops.layer_norm(t["x"], t["g"], t["b"], EPS, None)
    y2, xo2 = ops.layer_norm(t["x"], t["g"], t["b"], EPS)
    ln = torch.nn.LayerNorm(72, eps=EPS, device=device, dtype=BF16)
    with torch.no_grad():
        ln.weight.copy_(t["g"])
        ln.bias.copy_(t["b"])
        y3, xo3 = S.layer_norm(t["x"], ln, None)
    assert torch.equal(y, y2) and torch.equal(y, y3) and torch.equal(xo, t["x"]) and torch.equal(xo3, t["x"])
    assert verdict(c16, (y, xo), depth(info(c16))) <= 1
    t = {k: v.to(device) for k, v in make_inputs(c32).items() if v is not None}
    st = ops.ln_stats(t["x"], None)
    assert torch.equal(st, ops.ln_stats(t["x"])) and torch.equal(st, ops.ln_stats(t["x"], None, EPS))
    assert verdict(c32, (st,), depth(info(c32))) <= 1
    t = {k: v.to(device) for k, v in make_inputs(csp).items() if v is not None}
    ys = ops.layer_norm_split(t["x"], t["g"], t["b"], EPS, None)
    assert torch.equal(ys, ops.layer_norm_split(t["x"], t["g"], t["b"], EPS))
    assert verdict(csp, (ys,), depth(info(csp))) <= 1
    assert S.fallback_counts() == {}
