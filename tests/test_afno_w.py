"""The LayerNorm-fused AFNO W-transforms (csrc/spectral/afno_wfft.hip) per mode, channel and row, and the
device ``ln_stats_merge`` at any chunk count.

Six kernel instances (``torch.ops.amd_dft.afno_w_info`` names them): ``r2c_bf16``, ``r2c_f32``, ``c2r_bf16``,
``c2r_f32``, ``c2r_f32_split`` (split pairs + partial statistics) and ``c2r_bf16_part`` (partial statistics).

Reference: plain torch in fp64 written here (``x' = x + pre``, ``h = (x' - mean) rstd gamma + beta`` from the
GIVEN stats, ``torch.fft.rfft`` in complex128, a zero-padded half spectrum through ``irfft(norm="forward")``).

Comparison: per element.  ``|out - ref|`` is divided by the largest ``|ref|`` of the same (o, channel) column
along the transform axis and the worst element counts.  bf16 outputs: in bf16 ulps of that column maximum
(ulp = 2^(floor(log2 max) - 7)); fp32 outputs: as a plain ratio.

Bounds: twice the worst error measured on an MI355X over every comparison of the GPU tier below that runs a
kernel of afno_wfft.hip (the margin covers seeds and boxes; every comparison prints its figure).  Measured worst
-> bound, and the case that gave the worst:

    r2c_bf16       0.6073   -> 1.215   bf16 ulps  (2-D x, C = 192, no pre)
    r2c_f32        3.905e-7 -> 7.81e-7 of the max (O = 3, C = 192, pre)
    c2r_bf16       0.5536   -> 1.107   bf16 ulps  (one-hot (mode, re|im) probe)
    c2r_f32        2.468e-7 -> 4.94e-7 of the max (spectrum only, O = 3, C = 128)
    c2r_f32_split  2.468e-7 -> 4.94e-7 of the max (spectrum only, O = 3, C = 128)
    c2r_bf16_part  0.5373   -> 1.075   bf16 ulps  (O = 3, C = 64, pre)

The same bounds hold the CPU kernels, the fixed Stockham LayerNorm pass and the ATen route where a test goes there.

The mutation tests (CPU tier) prove every bound rejects: the spectral term dropped, mode 45 of one channel zeroed,
the two channels of a packed pair swapped in one mode, one mode conjugated, the stats of row o applied to row
o + 1, and one (o, slab) tile replaced by its neighbour's.
"""
import math

import pytest
import torch

from tensorrt_dft_plugins_amd.ops import spectral as S

ops = torch.ops.amd_dft
BF16, F32 = torch.bfloat16, torch.float32
L, KM = 180, 46
SCALE = 1 / math.sqrt(90 * 180)

# instance -> (op, dtype)
INSTANCES = {
    "r2c_bf16": ("r2c_ln", BF16), "r2c_f32": ("r2c_ln", F32),
    "c2r_bf16": ("c2r_ln_add", BF16), "c2r_f32": ("c2r_ln_add", F32),
    "c2r_f32_split": ("c2r_ln_add_split", F32), "c2r_bf16_part": ("c2r_ln_add_part", BF16),
}
# instance -> bound = 2 x the measured worst (module docstring); bf16 in ulps of the column max, fp32 a ratio
BOUND = {"r2c_bf16": 1.215, "r2c_f32": 7.81e-7, "c2r_bf16": 1.107, "c2r_f32": 4.94e-7, "c2r_f32_split": 4.94e-7,
         "c2r_bf16_part": 1.075}


# ------------------------------------------------------------------ fp64 reference
def ref_ln(x, stats, g, b, pre):
    xp = x.double() + (0 if pre is None else pre.double())
    st = stats.double().reshape(*x.shape[:-1], 2)
    return xp, (xp - st[..., :1]) * st[..., 1:] * g.double() + b.double()


def ref_r2c(x, stats, g, b, pre, scale):
    return torch.view_as_real(torch.fft.rfft(ref_ln(x, stats, g, b, pre)[1], dim=-2)[..., :KM, :] * scale)


def ref_spectral(Y, scale):
    """scale * irfft of the zero-padded half spectrum [..., KM, C, 2]; the imaginary part of mode 0 is ignored"""
    z = torch.view_as_complex(Y.double().contiguous())
    full = torch.zeros(*z.shape[:-2], L // 2 + 1, z.shape[-1], dtype=torch.complex128)
    full[..., :z.shape[-2], :] = z
    full[..., 0, :] = full[..., 0, :].real.to(torch.complex128)
    return scale * torch.fft.irfft(full, n=L, dim=-2, norm="forward")


def ref_c2r(Y, x, stats, g, b, pre, scale):
    xp, h = ref_ln(x, stats, g, b, pre)
    return ref_spectral(Y, scale) + xp + h


def col_err(out, ref, dtype, spec=False):
    """Worst |out - ref| over the column maximum of |ref| along the transform axis: bf16 in ulps of that
    maximum, fp32 as a ratio.  A column whose reference is all zero must be exactly zero."""
    out, ref = out.double().cpu(), ref.double()
    assert out.shape == ref.shape
    dims = (-3, -1) if spec else (-2,)  # spec: a spectrum [..., modes, C, 2]
    cmax = ref.abs().amax(dim=dims, keepdim=True)
    diff = (out - ref).abs()
    if not bool(torch.isfinite(out).all()):
        return math.inf
    zero = cmax == 0
    if bool((diff * zero).any()):
        return math.inf
    unit = torch.exp2(torch.floor(torch.log2(cmax.clamp_min(1e-300))) - 7) if dtype == BF16 else cmax
    return (diff / torch.where(zero, torch.ones_like(unit), unit)).max().item()


# ------------------------------------------------------------------ inputs
def make_inputs(lead, C, dtype, with_pre, seed=0, amp=20.0):
    """x O(1) around 0.5, its true LayerNorm statistics, gamma / beta / pre, and a spectrum whose inverse
    transform at SCALE weighs about as much as x' + LN(x') (amp 20)"""
    g = torch.Generator().manual_seed(1000 * seed + C + len(lead))
    x = (0.5 + torch.randn(*lead, L, C, generator=g)).to(dtype)
    pre = 0.3 * torch.randn(C, generator=g) if with_pre else None
    gam = 1 + 0.1 * torch.randn(C, generator=g)
    bet = 0.1 * torch.randn(C, generator=g)
    xp = x.double() + (0 if pre is None else pre.double())
    var, mean = torch.var_mean(xp, dim=-1, correction=0)
    stats = torch.stack([mean, torch.rsqrt(var + 1e-6)], -1).reshape(-1, 2).float()
    Y = (amp * torch.randn(*lead, KM, C, 2, generator=g)).to(dtype)
    return dict(x=x, stats=stats, g=gam, b=bet, pre=pre, Y=Y)


def call(inst, dev, t, scale=SCALE, out_mode=1):
    """The op of an instance on `dev`; returns its tuple of outputs"""
    d = lambda v: None if v is None else v.to(dev)  # noqa: E731
    op = INSTANCES[inst][0]
    if op == "r2c_ln":
        return (ops.r2c_ln(d(t["x"]), -2, scale, KM, d(t["stats"]), d(t["g"]), d(t["b"]), d(t["pre"]), t["x"].dtype),)
    a = (d(t["Y"]), -2, L, scale, d(t["x"]), d(t["stats"]), d(t["g"]), d(t["b"]), d(t["pre"]))
    if op == "c2r_ln_add":
        return (ops.c2r_ln_add(*a),)
    if op == "c2r_ln_add_split":
        return tuple(ops.c2r_ln_add_split(*a, out_mode))
    return tuple(ops.c2r_ln_add_part(*a))


def within(inst, err, what):
    """Print the figure (the bounds are set from these), then assert it"""
    print(f"afno_w worst {inst} {what}: {err:.4g}")
    assert err <= BOUND[inst], f"{inst} {what}: {err:.4g} > {BOUND[inst]}"


def check(inst, out, ref, what):
    within(inst, col_err(out, ref, INSTANCES[inst][1], inst.startswith("r2c")), what)


def reference(inst, t, scale=SCALE):
    a = (t["x"], t["stats"], t["g"], t["b"], t["pre"], scale)
    return ref_r2c(*a) if inst.startswith("r2c") else ref_c2r(t["Y"], *a)


def assert_route(inst, C):
    op, dt = INSTANCES[inst]
    info = ops.afno_w_info(op, L, C, KM, dt == BF16)
    assert info == f"wfft {inst} slabs={C // 64} stage={'fp16' if dt == BF16 else 'fp32'}", info


def chunk_stats64(y):
    """fp64 (mean, M2) of every 64-channel chunk of the rows of y [..., C] -> [rows, C / 64, 2]"""
    w = y.double().reshape(-1, y.shape[-1] // 64, 64)
    m = w.mean(-1)
    return torch.stack([m, (w - m.unsqueeze(-1)).pow(2).sum(-1)], -1)


def assert_part(part, y):
    """The epilogue's per-64-channel (mean, M2) against fp64 statistics of the stored output y.  The kernel sums
    d_i = y_i - y_0 in fp32 (u = 2^-24; 4 accumulators x 16 terms + 2 levels: <= 19 u sum|d| for S1, <= 20 u S2
    for S2) and takes mean = y_0 + S1 / 64, M2 = S2 - S1^2 / 64.  With D = max|d|: |mean error| <= u (19 D + 2
    |mean|), |M2 error| <= (20 + 38 + 2 + 1) 64 u D^2 < 2^-12 D^2.  A constant chunk (D = 0) has M2 = 0 exactly."""
    w = y.double().cpu().reshape(-1, y.shape[-1] // 64, 64)
    ref = chunk_stats64(y.cpu())
    D = (w - w[..., :1]).abs().amax(-1)
    u = 2.0 ** -24
    p = part.double().cpu()
    assert p.shape == ref.shape
    em = (p[..., 0] - ref[..., 0]).abs() - u * (19 * D + 2 * ref[..., 0].abs())
    e2 = (p[..., 1] - ref[..., 1]).abs() - 2.0 ** -12 * D * D
    assert em.max().item() <= 0, f"partial mean off by {em.max().item():.3e} beyond its bound"
    assert e2.max().item() <= 0, f"partial M2 off by {e2.max().item():.3e} beyond its bound"


def merge_ref(part, eps, shift=None):
    p = part.double()
    m, q = p[..., 0], p[..., 1]
    mean = m.mean(1)
    m2 = q.sum(1) + 64.0 * (m - mean.unsqueeze(1)).pow(2).sum(1)
    rstd = torch.rsqrt(m2 / (64.0 * p.shape[1]) + eps)
    if shift is not None:
        mean = mean - shift.double()[:, 0]
    return torch.stack([mean, rstd], 1)


def merge_inputs(rows, nc, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + rows * 64 + nc)
    part = torch.stack([0.5 + torch.randn(rows, nc, generator=g), 64 * (0.5 + torch.rand(rows, nc, generator=g))], -1)
    shift = torch.randn(rows, 2, generator=g)
    return part, shift


def assert_merge(st, part, shift):
    """fp32 merge against fp64: the mean is a sum of nc terms ((nc + 2) u max|mean_c|, one more rounding with a
    shift); the variance sums 2 nc positive O(1) terms whose d = mean_c - mean carries the mean's error, rsqrt
    halves the relative error and adds the device rsqrt's own: 4 (nc + 8) u relative."""
    nc, u = part.shape[1], 2.0 ** -24
    ref = merge_ref(part, 1e-6, shift)
    st = st.double().cpu()
    tol_m = (nc + 2) * u * part[..., 0].abs().amax(1).double() + (0 if shift is None else u * (ref[:, 0].abs() + shift[:, 0].abs().double()))
    assert bool(((st[:, 0] - ref[:, 0]).abs() <= tol_m).all()), ((st[:, 0] - ref[:, 0]).abs() - tol_m).max()
    assert bool(((st[:, 1] / ref[:, 1] - 1).abs() <= 4 * (nc + 8) * u).all()), (st[:, 1] / ref[:, 1] - 1).abs().max()


# ------------------------------------------------------------------ CPU tier
_MUT_CACHE = {}


def _mut_case():
    if not _MUT_CACHE:
        t = make_inputs((3,), 128, F32, True, seed=5)
        _MUT_CACHE.update(t=t, r2c=ref_r2c(t["x"], t["stats"], t["g"], t["b"], t["pre"], SCALE),
                          c2r=ref_c2r(t["Y"], t["x"], t["stats"], t["g"], t["b"], t["pre"], SCALE))
    return _MUT_CACHE


def _mutate(kind, r2c):
    """The reference with one defect"""
    c = _mut_case()
    t = dict(c["t"])
    ref = (c["r2c"] if r2c else c["c2r"]).clone()
    again = lambda: ref_r2c(t["x"], t["stats"], t["g"], t["b"], t["pre"], SCALE) if r2c else \
        ref_c2r(t["Y"], t["x"], t["stats"], t["g"], t["b"], t["pre"], SCALE)  # noqa: E731
    spec = ref if r2c else t["Y"].clone()  # the spectrum the defect touches: the R2C output or the C2R input
    if kind == "no_spectral":
        xp, h = ref_ln(t["x"], t["stats"], t["g"], t["b"], t["pre"])
        return xp + h
    if kind == "mode45_zero":
        spec[..., 45, 70, :] = 0
    elif kind == "pair_swap":
        spec[..., 17, [66, 67], :] = spec[..., 17, [67, 66], :]
    elif kind == "mode_conj":
        spec[..., 23, :, 1] = -spec[..., 23, :, 1]
    elif kind == "stats_row_shift":
        t["stats"] = t["stats"].reshape(3, L, 2).roll(1, 0).reshape(-1, 2)
        return again()
    elif kind == "tile_neighbour":
        ref[1, :, 0:64] = ref[1, :, 64:128]
        return ref
    else:
        raise AssertionError(kind)
    if r2c:
        return spec
    t["Y"] = spec
    return again()


MUTATIONS = ["no_spectral", "mode45_zero", "pair_swap", "mode_conj", "stats_row_shift", "tile_neighbour"]


@pytest.mark.parametrize("inst,kind", [(i, k) for i in INSTANCES for k in MUTATIONS
                                       if not (k == "no_spectral" and i.startswith("r2c"))])  # the R2C has no such term
def test_bound_rejects_mutation(inst, kind):
    """The comparison, fed the fp64 reference with one defect, exceeds the instance's bound (and accepts the
    reference rounded to the instance's output dtype)."""
    r2c = inst.startswith("r2c")
    dt = INSTANCES[inst][1]
    ref = _mut_case()["r2c" if r2c else "c2r"]
    assert col_err(ref.to(dt), ref, dt, r2c) <= BOUND[inst]
    assert col_err(_mutate(kind, r2c).to(dt), ref, dt, r2c) > BOUND[inst]


def test_mutation_case_sees_the_spectrum():
    c = _mut_case()
    t = c["t"]
    xp, h = ref_ln(t["x"], t["stats"], t["g"], t["b"], t["pre"])
    assert 0.5 <= (ref_spectral(t["Y"], SCALE).norm() / (xp + h).norm()).item() <= 2


@pytest.mark.parametrize("with_pre", [False, True])
@pytest.mark.parametrize("C", [64, 128, 192])
@pytest.mark.parametrize("lead", [(1,), (3,), ()], ids=["O1", "O3", "2d"])
@pytest.mark.parametrize("inst", list(INSTANCES))
def test_instance_cpu(inst, lead, C, with_pre):
    """The CPU kernels of the four ops against the same reference, comparison and bounds"""
    dt = INSTANCES[inst][1]
    t = make_inputs(lead, C, dt, with_pre, seed=1)
    ref = reference(inst, t)
    outs = call(inst, "cpu", t)
    assert outs[0].dtype == dt
    check(inst, outs[0], ref, "cpu")
    y = outs[0]
    if inst == "c2r_f32_split":
        assert torch.equal(outs[1], ops.split_bf16(y.reshape(-1, C) - t["stats"][:, :1], True))
        assert_part(outs[2], y)
        for mode in (0, 2):
            o2 = call(inst, "cpu", t, out_mode=mode)
            assert torch.equal(o2[1], outs[1]) and torch.equal(o2[2], outs[2])
            assert o2[0].numel() == (0 if mode == 0 else y.numel())
    if inst == "c2r_bf16_part":
        assert_part(outs[1], y)


def test_mode0_imag_ignored_cpu():
    t = make_inputs((1,), 64, F32, False, seed=2)
    a = call("c2r_f32", "cpu", t)[0]
    t["Y"][..., 0, :, 1] = 7.0
    assert torch.equal(call("c2r_f32", "cpu", t)[0], a)


@pytest.mark.parametrize("use_shift", [False, True])
@pytest.mark.parametrize("nc", [1, 2, 3, 12, 64])
def test_ln_stats_merge_cpu(nc, use_shift):
    part, shift = merge_inputs(257, nc)
    assert_merge(ops.ln_stats_merge(part, 1e-6, shift if use_shift else None), part, shift if use_shift else None)


def test_afno_w_info_routes():
    info = ops.afno_w_info
    for inst, (op, dt) in INSTANCES.items():
        for C in (64, 128, 192, 768):
            assert_route(inst, C)
    # outside the specialised shape: bf16 on the fixed Stockham LayerNorm pass where one is compiled for the
    # length and the channel count is even; fp32, odd channel counts and other lengths through ATen
    assert info("r2c_ln", 180, 32, 46, True).startswith("stockham L=180 ")
    assert info("c2r_ln_add", 180, 64, 40, True).startswith("stockham L=180 ")
    assert info("r2c_ln", 90, 64, 46, True).startswith("stockham L=90 ")
    assert info("r2c_ln", 180, 33, 46, True).startswith("aten ")
    assert info("r2c_ln", 180, 32, 46, False).startswith("aten ")
    assert info("c2r_ln_add", 96, 64, 40, True).startswith("aten ")
    assert info("c2r_ln_add_part", 180, 64, 40, True).startswith("aten epilogue; c2r_ln_add: stockham L=180 ")
    assert info("c2r_ln_add_split", 180, 64, 40, False).startswith("aten epilogue; c2r_ln_add: aten ")
    assert info("c2r_ln_add_split", 180, 64, 46, True).startswith("none ")
    assert info("c2r_ln_add_part", 180, 64, 46, False).startswith("none ")
    assert info("c2r_ln_add_part", 180, 96, 46, True).startswith("none ")
    with pytest.raises(RuntimeError, match="op must be"):
        info("c2r", 180, 64, 46, True)


# ------------------------------------------------------------------ fp64 images of the fp16-staged values
def staged_r2c(h):
    """|components| of what the bf16 R2C stages in fp16 for h [L, C]: the 12-point sums of pass 0 (twiddled) and
    the unscaled 180-point sums of the packed pairs z = h_c + i h_{c+1}"""
    z = torch.complex(h[:, 0::2].double(), h[:, 1::2].double())
    s0 = torch.fft.fft(z.reshape(12, 15, -1), dim=0)  # n = n2 + 15 n1 -> [k1, n2]
    k1, n2 = torch.arange(12.0, dtype=torch.float64).reshape(12, 1, 1), torch.arange(15.0, dtype=torch.float64).reshape(1, 15, 1)
    s0 = s0 * torch.polar(torch.ones(12, 15, 1, dtype=torch.float64), -2 * math.pi * k1 * n2 / L)
    Z = torch.fft.fft(z, dim=0)
    return torch.cat([torch.view_as_real(s0).reshape(-1), torch.view_as_real(Z).reshape(-1)]).abs()


def staged_c2r(Y):
    """|components| of what the bf16 C2R stages in fp16 for a spectrum Y [KM, C, 2]: the twiddled 12-point sums of
    the Hermitian-assembled packed spectrum Z[n] = conj(X_c[n] + i X_{c+1}[n])"""
    X = torch.view_as_complex(Y.double().contiguous())
    X[0] = X[0].real.to(torch.complex128)
    full = torch.zeros(L, X.shape[1], dtype=torch.complex128)
    full[:KM] = X
    full[L - KM + 1:] = X[1:].conj().flip(0)
    z = (full[:, 0::2] + 1j * full[:, 1::2]).conj()
    s0 = torch.fft.fft(z.reshape(12, 15, -1), dim=0)
    k1, n2 = torch.arange(12.0, dtype=torch.float64).reshape(12, 1, 1), torch.arange(15.0, dtype=torch.float64).reshape(1, 15, 1)
    s0 = s0 * torch.polar(torch.ones(12, 15, 1, dtype=torch.float64), -2 * math.pi * k1 * n2 / L)
    return torch.view_as_real(s0).reshape(-1).abs()


R2C_STAGE_MAX = 65504 / (180 * math.sqrt(2))  # |LN output|, afno_wfft.hip header
C2R_STAGE_MAX = 65504 / (12 * math.sqrt(2))   # |spectrum component|
STAGE_MIN = 2.0 ** -16                         # both


def _plain_ln(t):
    """LayerNorm that passes x through: stats (0, 1), gamma 1, beta 0, no pre"""
    C = t["x"].shape[-1]
    t.update(stats=torch.tensor([0.0, 1.0]).repeat(t["x"].numel() // C, 1), g=torch.ones(C), b=torch.zeros(C), pre=None)
    return t


def stage_case_r2c_top():
    """|h| = 64 <= a quarter of the bound; pair (0, 1) of row 0 carries sign(cos), sign(sin) of mode 1, which sums to
    64 * sum(|cos| + |sin|) = 64 * 229 in one component of Z[1]; pair (2, 3) is constant (180 * 64 in mode 0)"""
    t = _plain_ln(make_inputs((1,), 64, BF16, False, seed=3))
    th = 2 * math.pi * torch.arange(L) / L
    x = t["x"].float().clamp(-1, 1) * 64
    x[0, :, 0] = 64 * torch.where(torch.cos(th) >= 0, 1.0, -1.0)
    x[0, :, 1] = 64 * torch.where(torch.sin(th) >= 0, 1.0, -1.0)
    x[0, :, 2:4] = 64
    t["x"] = x.to(BF16)
    return t


def stage_case_c2r_top():
    """|component| = 960 <= a quarter of the bound; the six modes a pass-0 sum of n2 = 1, k1 = 1 reads (1, 16, 31 and
    the mirrors of 44, 29, 14) are phased to add up in its real part"""
    t = _plain_ln(make_inputs((1,), 64, BF16, False, seed=4))
    t["x"] = torch.zeros_like(t["x"])
    a = 960.0
    Y = t["Y"].float().clamp(-1, 1) * a
    for n1 in (0, 1, 2, 9, 10, 11):
        n = 1 + 15 * n1
        phi = 2 * math.pi * (n1 / 12 + 1 / L)  # the sum adds Z[n] e^{-i phi}: Z = 2a (sign cos phi, sign sin phi)
        zr, zi = 2 * a * math.copysign(1, math.cos(phi)), 2 * a * math.copysign(1, math.sin(phi))
        if n <= L // 2:  # Z = conj(A + iB) = (A.re - B.im, -(A.im + B.re))
            Y[0, n, 0] = torch.tensor([zr / 2, -zi / 2])
            Y[0, n, 1] = torch.tensor([-zi / 2, -zr / 2])
        else:            # mode k = L - n: Z = A - iB = (A.re + B.im, A.im - B.re)
            Y[0, L - n, 0] = torch.tensor([zr / 2, zi / 2])
            Y[0, L - n, 1] = torch.tensor([-zi / 2, zr / 2])
    t["Y"] = Y.to(BF16)
    return t


def test_staging_cases_reach_their_magnitudes():
    """On the fp64 reference: the inputs of the staging-range tests stay inside the documented amplitudes and their
    staged sums come to within 15 % of a quarter of fp16's maximum (top) / stay at fp16's subnormal edge (bottom)."""
    t = stage_case_r2c_top()
    assert t["x"].abs().max().item() <= R2C_STAGE_MAX / 4
    assert 0.85 * 65504 / 4 <= staged_r2c(t["x"][0]).max().item() <= 65504 / 4
    t = stage_case_c2r_top()
    assert t["Y"].abs().max().item() <= C2R_STAGE_MAX / 4
    assert 0.85 * 65504 / 4 <= staged_c2r(t["Y"][0]).max().item() <= 65504 / 4
    t = stage_case_bottom()
    assert t["x"].abs().max().item() == 4 * STAGE_MIN and t["Y"].abs().max().item() == 4 * STAGE_MIN
    for o in range(t["x"].shape[0]):
        assert 0 < staged_r2c(t["x"][o]).max().item() <= 2 * 4 * STAGE_MIN  # at most two lone inputs in one staged value
        assert 0 < staged_c2r(t["Y"][o]).max().item() <= 2 * 2 * 4 * STAGE_MIN


def stage_case_bottom():
    """Lone inputs of amplitude 4 * 2^-16 = 2^-14 (fp16's smallest normal): row o has one token (R2C) / one spectrum
    component (C2R) of one packed channel pair set, so every staged value is that input times a twiddle -- fp16 subnormals"""
    O = 8
    t = _plain_ln(make_inputs((O,), 64, BF16, False, seed=6))
    x = torch.zeros(O, L, 64)
    Y = torch.zeros(O, KM, 64, 2)
    for o in range(O):
        c = (10 * o) % 64  # both channels of a packed pair: neither column's reference is all zero
        x[o, 23 * o + 1, c:c + 2] = 4 * STAGE_MIN
        Y[o, (6 * o + 1) % KM, c:c + 2, o % 2] = 4 * STAGE_MIN
    t.update(x=x.to(BF16), Y=Y.to(BF16))
    return t


# ------------------------------------------------------------------ GPU tier
def _gpu_call(inst, device, t, scale=SCALE, out_mode=1):
    S.fallback_reset()
    outs = call(inst, device, t, scale, out_mode)
    assert S.fallback_counts() == {}
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("with_pre", [False, True])
@pytest.mark.parametrize("C", [64, 128, 192])
@pytest.mark.parametrize("lead", [(1,), (3,), ()], ids=["O1", "O3", "2d"])
@pytest.mark.parametrize("inst", list(INSTANCES))
def test_instance_gpu(device, inst, lead, C, with_pre):
    """Every instance at O in {1, 3} and a 2-D x, 1 to 3 slabs, with and without pre: worst element within the bound,
    the route asserted, no fallback; the split instance in all three out_modes with its pairs bit-exact, and both
    statistics epilogues against fp64 statistics of the stored output."""
    dt = INSTANCES[inst][1]
    assert_route(inst, C)
    t = make_inputs(lead, C, dt, with_pre, seed=1)
    ref = reference(inst, t)
    outs = _gpu_call(inst, device, t)
    y = outs[0]
    assert y.dtype == dt and y.shape == ref.shape
    check(inst, y, ref, f"lead={lead} C={C} pre={int(with_pre)}")
    if inst == "c2r_f32_split":
        st = t["stats"].to(device)
        assert torch.equal(outs[1], ops.split_bf16(y.reshape(-1, C) - st[:, :1], True))
        assert_part(outs[2], y)
        o0 = _gpu_call(inst, device, t, out_mode=0)
        o2 = _gpu_call(inst, device, t, out_mode=2)
        assert o0[0].numel() == 0 and o2[0].dtype == BF16 and o2[0].shape == (y.numel() // C, C)
        for o in (o0, o2):
            assert torch.equal(o[1], outs[1]) and torch.equal(o[2], outs[2])
        # pairs + lo2 + mean give the fp32 output back to ~2^-27 of |y - mean| (the bound of the 768-channel test)
        z = (y.reshape(-1, C) - st[:, :1]).cpu()
        back = S.unsplit_bf16(outs[1].cpu()) + o2[0].cpu().float()
        assert (back - z).abs().max() <= 2 ** -26 * z.abs().max(), (back - z).abs().max()
    if inst == "c2r_bf16_part":
        assert_part(outs[1], y)
        assert torch.equal(y, _gpu_call("c2r_bf16", device, t)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("inst", [i for i in INSTANCES if i.startswith("c2r")])
def test_c2r_term_isolation_gpu(device, inst):
    """Spectrum only (the output is exactly scale * irfft(Y)), addends only (Y = 0), and both with the spectral term
    weighing between half and twice the addends -- asserted on the reference."""
    dt = INSTANCES[inst][1]
    t = make_inputs((3,), 128, dt, True, seed=7)
    xp, h = ref_ln(t["x"], t["stats"], t["g"], t["b"], t["pre"])
    assert 0.5 <= (ref_spectral(t["Y"], SCALE).norm() / (xp + h).norm()).item() <= 2
    check(inst, _gpu_call(inst, device, t)[0], reference(inst, t), "both terms")
    only_add = dict(t, Y=torch.zeros_like(t["Y"]))
    check(inst, _gpu_call(inst, device, only_add)[0], xp + h, "addends only")
    only_spec = _plain_ln(dict(t, x=torch.zeros_like(t["x"])))
    check(inst, _gpu_call(inst, device, only_spec)[0], ref_spectral(t["Y"], SCALE), "spectrum only")


@pytest.mark.gpu
@pytest.mark.parametrize("inst", ["r2c_bf16", "r2c_f32"])
def test_r2c_one_hot_gpu(device, inst):
    """Row o holds a single 1 at w = o in channel o % 64: that channel is scale * e^{-2 pi i k o / 180}, its pair
    partner within the bound of zero, every other channel exactly zero."""
    dt = INSTANCES[inst][1]
    t = _plain_ln(make_inputs((L,), 64, dt, False))
    x = torch.zeros(L, L, 64)
    o = torch.arange(L)
    x[o, o, o % 64] = 1
    t["x"] = x.to(dt)
    out = _gpu_call(inst, device, t, scale=0.5)[0].double().cpu()
    k = torch.arange(KM, dtype=torch.float64)
    unit = 2.0 ** -8 if dt == BF16 else 0.5  # the column max is 0.5: its bf16 ulp, or itself
    hot = partner = 0.0
    for r in range(L):
        c = r % 64
        want = torch.view_as_real(0.5 * torch.polar(torch.ones(KM, dtype=torch.float64), -2 * math.pi * k * r / L))
        hot = max(hot, ((out[r, :, c] - want).abs().max() / unit).item())
        partner = max(partner, (out[r, :, c ^ 1].abs().max() / unit).item())
        rest = torch.ones(64, dtype=torch.bool)
        rest[[c, c ^ 1]] = False
        assert not out[r][:, rest].any()
    within(inst, hot, "one-hot channel")
    within(inst, partner, "one-hot pair partner")


@pytest.mark.gpu
@pytest.mark.parametrize("inst", ["c2r_bf16", "c2r_f32"])
def test_c2r_one_hot_gpu(device, inst):
    """One row per (mode, re | im), x = 0: cosine / minus-sine patterns with the Hermitian factor 2 for k > 0; the
    imaginary part of mode 0 contributes exactly nothing, on the device and in the CPU op."""
    dt = INSTANCES[inst][1]
    O = 2 * KM
    t = _plain_ln(make_inputs((O,), 64, dt, False))
    t["x"] = torch.zeros(O, L, 64, dtype=dt)
    Y = torch.zeros(O, KM, 64, 2)
    o = torch.arange(O)
    Y[o, o // 2, (3 * o) % 64, o % 2] = 1
    t["Y"] = Y.to(dt)
    out = _gpu_call(inst, device, t, scale=0.5)[0].double().cpu()
    cpu = call(inst, "cpu", t, scale=0.5)[0].double()
    w = torch.arange(L, dtype=torch.float64)
    hot = partner = 0.0
    for r in range(O):
        k, im, c = r // 2, r % 2, (3 * r) % 64
        th = 2 * math.pi * k * w / L
        want = 0.5 * (1 if k == 0 else 2) * (-torch.sin(th) if im else torch.cos(th))
        if k == 0 and im:
            assert not out[r].any() and not cpu[r].any()
            continue
        hot = max(hot, col_err(out[r, :, c:c + 1], want.unsqueeze(1), dt))
        rest = torch.ones(64, dtype=torch.bool)
        rest[[c, c ^ 1]] = False
        assert not out[r][:, rest].any()
        # the column max is 0.5 or 1: a power of two, whose bf16 ulp is 2^-7 of it
        partner = max(partner, (out[r, :, c ^ 1].abs().max() / want.abs().max()).item() * (2.0 ** 7 if dt == BF16 else 1))
    within(inst, hot, "one-hot (mode, re|im)")
    within(inst, partner, "one-hot pair partner")


def _slice_tile(t, o, s):
    cs = slice(64 * s, 64 * s + 64)
    return dict(x=t["x"][o:o + 1, :, cs].contiguous(), stats=t["stats"].reshape(-1, L, 2)[o].contiguous(),
                g=t["g"][cs].contiguous(), b=t["b"][cs].contiguous(),
                pre=None if t["pre"] is None else t["pre"][cs].contiguous(), Y=t["Y"][o:o + 1, :, cs].contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("inst", list(INSTANCES))
def test_tile_independence_gpu(device, inst):
    """O = 3, C = 192 equals, bit for bit, its nine (o, slab) problems run alone at O = 1, C = 64 -- every output."""
    dt = INSTANCES[inst][1]
    t = make_inputs((3,), 192, dt, True, seed=8)
    modes = (1, 2) if inst == "c2r_f32_split" else (1,)
    for mode in modes:
        big = [v.cpu() for v in _gpu_call(inst, device, t, out_mode=mode)]
        for o in range(3):
            for s in range(3):
                small = [v.cpu() for v in _gpu_call(inst, device, _slice_tile(t, o, s), out_mode=mode)]
                cs = slice(64 * s, 64 * s + 64)
                if inst.startswith("r2c"):
                    assert torch.equal(big[0][o, :, cs], small[0][0])
                    continue
                first = big[0].reshape(3, L, 192)[o, :, cs]  # out, or lo2 [tokens, C]
                assert torch.equal(first, small[0].reshape(L, 64))
                if inst == "c2r_f32_split":
                    assert torch.equal(big[1].reshape(3, L, 3, 128)[o, :, s], small[1])
                    assert torch.equal(big[2].reshape(3, L, 3, 2)[o, :, s], small[2].reshape(L, 2))
                if inst == "c2r_bf16_part":
                    assert torch.equal(big[1].reshape(3, L, 3, 2)[o, :, s], small[1].reshape(L, 2))


def _embedded(v, device, offset):
    """v as a contiguous view `offset` elements into a larger NaN-filled device buffer (>= 64 elements either side)"""
    buf = torch.full((v.numel() + 256,), math.nan, dtype=v.dtype, device=device)
    view = buf[offset:offset + v.numel()].view(v.shape)
    view.copy_(v)
    return view


def _call_embedded(inst, device, t, offsets):
    """call() with each named input embedded at its offset (elements); all others plain device tensors"""
    e = {k: (None if v is None else _embedded(v, device, offsets[k]) if k in offsets else v.to(device)) for k, v in t.items()}
    return _gpu_call(inst, device, e)


@pytest.mark.gpu
@pytest.mark.parametrize("inst", list(INSTANCES))
def test_poisoned_surroundings_gpu(device, inst):
    """Every input a 16-byte-aligned view into a larger NaN-filled buffer: outputs bit-identical to the stand-alone run"""
    dt = INSTANCES[inst][1]
    t = make_inputs((3,), 128, dt, True, seed=9)
    plain = _gpu_call(inst, device, t)
    inside = _call_embedded(inst, device, t, {k: 64 for k in t})
    for a, b in zip(plain, inside):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("inst", list(INSTANCES))
def test_misaligned_views_gpu(device, inst):
    """Each input in turn a contiguous view ONE element into a larger buffer (not 16-byte aligned: the ops copy it):
    results bit-identical to the aligned call"""
    dt = INSTANCES[inst][1]
    t = make_inputs((2,), 64, dt, True, seed=10)
    plain = _gpu_call(inst, device, t)
    for name in ("x", "stats", "g", "b", "pre") + (() if inst.startswith("r2c") else ("Y",)):
        off = _call_embedded(inst, device, t, {name: 1})
        for a, b in zip(plain, off):
            assert torch.equal(a, b), name


@pytest.mark.gpu
@pytest.mark.parametrize("inst", ["c2r_f32_split", "c2r_bf16_part"])
def test_part_epilogue_gpu(device, inst):
    """The per-64-channel (mean, M2) of both statistics epilogues, before any merge, against fp64 statistics of the
    stored output: rows with |mean| / std = 100, and a slab of constant values (M2 = 0 exactly)."""
    dt = INSTANCES[inst][1]
    t = make_inputs((3,), 192, dt, True, seed=11)
    x = t["x"].float()
    x[1] += 100.0  # std 1 around 100
    x[2, :, 128:] = 3.0
    t["x"] = x.to(dt)
    t["g"][128:] = 0  # LN(x') = beta there
    t["b"][128:] = 0.25
    t["pre"][128:] = 0.5
    t["Y"][2, :, 128:] = 0
    xp = t["x"].double() + t["pre"].double()
    var, mean = torch.var_mean(xp, dim=-1, correction=0)
    t["stats"] = torch.stack([mean, torch.rsqrt(var + 1e-6)], -1).reshape(-1, 2).float()
    ratio = (mean[1].abs() / var[1].sqrt()).min().item()
    assert ratio > 50, ratio
    outs = _gpu_call(inst, device, t)
    y, part = outs[0], outs[-1]
    check(inst, y, reference(inst, t), "|mean|/std = 100 rows, constant slab")
    assert_part(part, y)
    const = part.reshape(3, L, 3, 2)[2, :, 2].cpu()
    assert torch.equal(const[:, 1], torch.zeros(L)) and torch.equal(const[:, 0], torch.full((L,), 3.75))


@pytest.mark.gpu
@pytest.mark.parametrize("use_shift", [False, True])
@pytest.mark.parametrize("rows", [1, 255, 257])
@pytest.mark.parametrize("nc", [1, 2, 3, 12, 64])
def test_ln_stats_merge_gpu(device, nc, rows, use_shift):
    """The device merge at odd and even chunk counts, one row to more than one workgroup, against an fp64 merge and the
    CPU op"""
    part, shift = merge_inputs(rows, nc)
    sh = shift if use_shift else None
    st = ops.ln_stats_merge(part.to(device), 1e-6, None if sh is None else sh.to(device))
    assert st.shape == (rows, 2)
    assert_merge(st, part, sh)
    cpu = ops.ln_stats_merge(part, 1e-6, sh)
    u = 2.0 ** -24
    assert torch.allclose(st.cpu().double(), cpu.double(), rtol=8 * (nc + 8) * u, atol=2 * (nc + 3) * u * 4.5)


@pytest.mark.gpu
def test_c192_block_statistics_gpu(device):
    """Embed width 192 (three 64-channel chunks) through the bf16 statistics epilogue and the device merge: the
    path that raised "needs an even chunk count" on the device only"""
    t = make_inputs((2,), 192, BF16, True, seed=12)
    y, part = _gpu_call("c2r_bf16_part", device, t)
    st = ops.ln_stats_merge(part, 1e-6).cpu().double()
    var, mean = torch.var_mean(y.double().cpu().reshape(-1, 192), dim=-1, correction=0)
    assert torch.allclose(st[:, 0], mean, rtol=0, atol=2e-6 * (1 + mean.abs().max().item()))
    assert torch.allclose(st[:, 1], torch.rsqrt(var + 1e-6), rtol=2e-5, atol=0)


@pytest.mark.gpu
def test_staging_range_gpu(device):
    """bf16 instances at a quarter of the documented fp16 staging maxima and at four times the documented lower
    amplitude (spectrum-only form): finite and within the bound (test_staging_cases_reach_their_magnitudes shows the
    staged sums really get there).  Nothing runs above the upper bound."""
    t = stage_case_r2c_top()
    check("r2c_bf16", _gpu_call("r2c_bf16", device, t, scale=1.0)[0], reference("r2c_bf16", t, 1.0), "staging top")
    t = stage_case_c2r_top()
    for inst in ("c2r_bf16", "c2r_bf16_part"):
        check(inst, _gpu_call(inst, device, t, scale=1.0)[0], ref_spectral(t["Y"], 1.0), "staging top")
    t = stage_case_bottom()
    check("r2c_bf16", _gpu_call("r2c_bf16", device, t, scale=1.0)[0], reference("r2c_bf16", t, 1.0), "staging bottom")
    t["x"] = torch.zeros_like(t["x"])
    for inst in ("c2r_bf16", "c2r_bf16_part"):
        check(inst, _gpu_call(inst, device, t, scale=1.0)[0], ref_spectral(t["Y"], 1.0), "staging bottom")


@pytest.mark.gpu
def test_routes_outside_the_specialised_shape_gpu(device):
    """bf16 off the specialised shape runs the fixed Stockham LayerNorm pass (smallest reachable: two channels), checked
    with the same reference and comparison and not counted as a fallback; fp32 there takes ATen and is counted."""
    g = torch.Generator().manual_seed(13)
    for C, km in ((2, 46), (64, 40)):
        assert ops.afno_w_info("r2c_ln", L, C, km, True).startswith("stockham ")
        assert ops.afno_w_info("c2r_ln_add", L, C, km, True).startswith("stockham ")
        x = (0.5 + torch.randn(2, L, C, generator=g)).to(BF16)
        var, mean = torch.var_mean(x.double(), dim=-1, correction=0)
        st = torch.stack([mean, torch.rsqrt(var + 1e-6)], -1).reshape(-1, 2).float()
        gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        Y = (20 * torch.randn(2, km, C, 2, generator=g)).to(BF16)
        d = lambda v: v.to(device)  # noqa: E731
        S.fallback_reset()
        X = ops.r2c_ln(d(x), -2, SCALE, km, d(st), d(gam), d(bet), None, BF16)
        y = ops.c2r_ln_add(d(Y), -2, L, SCALE, d(x), d(st), d(gam), d(bet), None)
        assert S.fallback_counts() == {}
        xp, h = ref_ln(x, st, gam, bet, None)
        Xref = torch.view_as_real(torch.fft.rfft(h, dim=-2)[..., :km, :] * SCALE)
        z = torch.zeros(2, L // 2 + 1, C, dtype=torch.complex128)
        z[:, :km] = torch.view_as_complex(Y.double())
        yref = SCALE * torch.fft.irfft(z, n=L, dim=-2, norm="forward") + xp + h
        within("r2c_bf16", col_err(X, Xref, BF16, True), f"stockham C={C} km={km}")
        within("c2r_bf16", col_err(y, yref, BF16), f"stockham C={C} km={km}")
    assert ops.afno_w_info("r2c_ln", L, 32, KM, False).startswith("aten ")
    t = make_inputs((1,), 32, F32, False, seed=14)
    S.fallback_reset()
    X = call("r2c_f32", device, t)[0]
    y = call("c2r_f32", device, t)[0]
    fc = S.fallback_counts()
    assert fc.get("r2c_ln", 0) >= 1 and fc.get("c2r_ln_add", 0) >= 1, fc
    S.fallback_reset()
    check("r2c_f32", X, reference("r2c_f32", t), "aten C=32")
    check("c2r_f32", y, reference("c2r_f32", t), "aten C=32")
