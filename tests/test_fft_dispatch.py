"""Every reachable FFT kernel configuration and tile shape, checked instead of assumed.

Which kernel a transform pass runs depends on its shape: ``prepare_fixed`` scores the compile-time
configurations of ``AMD_DFT_FIXED_CONFIGS`` by workgroup and wave counts, ``choose_tiling`` gives the
generic runtime-radix kernel a tile of ``T = 1 << logT`` signals.  ``torch.ops.amd_dft.fft_pass_info``
answers on the host, from the functions the launch uses, what a pass would launch.

* CPU tier: the ``CASES`` table below hits what it claims to hit, every shipped fixed configuration is
  either hit or proven dead by a brute-force sweep of the selection score (``UNREACHABLE``), and the
  generic kernel's tile widths, ragged last tiles and unpaired last real signals are all present.
* GPU tier: every case against ``torch.fft`` in float64 with a per-signal metric, plus pruned windows,
  ``c2r_add`` addends, multi-pass radix positions and inputs that are not aligned to a vector.
"""
import re
from collections import namedtuple

import pytest
import torch

import tensorrt_dft_plugins_amd as tdp
from helpers import long_fft_tol, per_signal_rel_l2, rel_l2

OPS = torch.ops.amd_dft

F32, BF16 = "f32", "bf16"
DT = {F32: torch.float32, BF16: torch.bfloat16}
ONE = ((F32, F32),)
ALL4 = ((F32, F32), (BF16, F32), (F32, BF16), (BF16, BF16))  # launch_dt's four instantiations

# kind, logical input shape (no trailing re/im dim; c2r: the stored half spectrum), transformed axis,
# transform length, (input, output) dtype pairs, expected substring of fft_pass_info
Case = namedtuple("Case", "kind shape axis n dtypes expect")


def _fixed(L, cols, TP, T, extra=""):
    return f"fixed L={L} cols={cols} TP={TP} T={T} " + extra


def _generic(L, cols, logT):
    return re.compile(rf"generic L={L} radices=\[[\d,]+\] cols={cols} logT={logT} ")


def _c2r(shape, axis, n, dtypes, expect):
    s = list(shape)
    s[axis] = n // 2 + 1
    return Case("c2r", tuple(s), axis, n, dtypes, expect)


CASES = [
    # ---- generic kernel, row-like: a tile is doubled only while >= 1024 workgroups remain
    Case("r2c", (2051, 12), 1, 12, ONE, _generic(12, 0, 0)),
    Case("r2c", (4101, 12), 1, 12, ONE, _generic(12, 0, 1)),  # 2051 pairs, the last one unpaired and alone in its tile
    # bf16 outputs on lines long enough that one rounding flip against the bf16-rounded reference
    # (2^-7 of one element) stays below the bound
    Case("r2c", (4101, 143), 1, 143, ALL4, _generic(143, 0, 1)),
    _c2r((4101, 14), 1, 14, ONE, _generic(14, 0, 1)),
    Case("c2c", (4101, 22), 1, 22, ONE, _generic(22, 0, 2)),  # 4101 = 1025 * 4 + 1
    Case("r2c", (16375, 12), 1, 12, ONE, _generic(12, 0, 3)),  # 8188 pairs = 1023 * 8 + 4, the last unpaired
    _c2r((16375, 14), 1, 14, ONE, _generic(14, 0, 3)),
    Case("r2c", (130951, 12), 1, 12, ONE, _generic(12, 0, 6)),  # 65476 pairs = 1023 * 64 + 4
    _c2r((130951, 14), 1, 14, ONE, _generic(14, 0, 6)),
    Case("c2c", (130951, 12), 1, 12, ONE, _generic(12, 0, 6)),  # 130951 = 2046 * 64 + 7
    # ---- generic kernel, column-like: up to T = 8 while >= 128 workgroups remain, wider from 1024
    Case("c2c", (16, 48, 17), 1, 48, ALL4, _generic(48, 1, 1)),
    Case("r2c", (16, 48, 33), 1, 48, ONE, _generic(48, 1, 1)),  # 17 pairs, the last unpaired
    Case("c2c", (40, 143, 27), 1, 143, ONE, _generic(143, 1, 3)),
    _c2r((40, 143, 53), 1, 143, ONE, _generic(143, 1, 3)),  # 27 pairs = 3 * 8 + 3, the last unpaired
    Case("c2c", (128, 22, 130), 1, 22, ONE, _generic(22, 1, 4)),  # 130 = 8 * 16 + 2
    # ---- 720-point columns: the three live configurations, all three kinds
    Case("c2c", (9, 720, 305), 1, 720, ONE, _fixed(720, 1, 45, 16)),  # 20 tiles per outer index, the last holds one column
    Case("r2c", (9, 720, 609), 1, 720, ONE, _fixed(720, 1, 45, 16)),
    Case("c2c", (2, 720, 721), 1, 720, ONE, _fixed(720, 1, 90, 8)),
    _c2r((1, 720, 1333), 1, 720, ONE, _fixed(720, 1, 90, 4)),
    # ---- 90 / 180 columns (channel-last): an odd channel count kills the paired-vector variant
    Case("r2c", (2, 90, 23), 1, 90, ONE, re.compile(_fixed(90, 1, 10, 16) + ".* pairvec=0")),
    Case("r2c", (2, 90, 24), 1, 90, ALL4, re.compile(_fixed(90, 1, 10, 16) + ".* pairvec=1")),
    _c2r((2, 90, 23), 1, 90, ONE, re.compile(_fixed(90, 1, 10, 16) + ".* pairvec=0")),
    _c2r((2, 90, 24), 1, 90, ONE, re.compile(_fixed(90, 1, 10, 16) + ".* pairvec=1")),
    Case("r2c", (2, 180, 23), 1, 180, ONE, re.compile(_fixed(180, 1, 15, 32) + ".* pairvec=0")),
    Case("r2c", (2, 180, 64), 1, 180, ONE, re.compile(_fixed(180, 1, 15, 16) + ".* pairvec=1")),
    _c2r((2, 180, 23), 1, 180, ALL4, re.compile(_fixed(180, 1, 15, 32) + ".* pairvec=0")),
    _c2r((2, 180, 24), 1, 180, ONE, re.compile(_fixed(180, 1, 15, 32) + ".* pairvec=1")),
    Case("c2c", (2, 180, 23), 1, 180, ALL4, _fixed(180, 1, 15, 16)),
    Case("c2c", (2, 90, 23), 1, 90, ONE, _fixed(90, 1, 10, 16)),
]
# ---- row kernels at an odd batch (an unpaired last signal, a ragged tile where T > 1)
for _L, _TP, _T in [(256, 16, 4), (512, 64, 2), (720, 90, 2), (1024, 128, 1), (2048, 256, 1), (1440, 288, 1)]:
    CASES += [Case("r2c", (3, _L), 1, _L, ONE, _fixed(_L, 0, _TP, _T)),
              _c2r((3, _L), 1, _L, ONE, _fixed(_L, 0, _TP, _T)),
              Case("c2c", (3, _L), 1, _L, ONE, _fixed(_L, 0, _TP, _T))]

# (L, cols, TP, T) of shipped configurations that never win the selection score
UNREACHABLE = {
    (720, 1, 90, 2): "(90, 4) has at least as many waves whenever (90, 2) passes a threshold, and a higher tie-break",
    (720, 1, 45, 8): "(90, 8) covers the same tiles with twice the waves and a higher tie-break",
    (720, 1, 45, 4): "(90, 4) covers the same tiles with twice the waves and a higher tie-break",
}
# (L, cols, TP, T, radices): selected only by a tuning build's radix override (MI_DFT_FFT_RADICES),
# so they cannot run in the shipped library
TUNING_ONLY = {
    (1440, 0, 144, 1, "10,12,12"), (720, 0, 30, 2, "24,30"), (720, 1, 30, 4, "24,30"), (720, 1, 30, 8, "24,30"),
}

GENERIC_ROW_LOGT = {0, 1, 2, 3, 6}
GENERIC_COL_LOGT = {1, 3, 4}


def _case_id(c):
    return f"{c.kind}-{'x'.join(map(str, c.shape))}-n{c.n}"


def _info(c, tin=F32, tout=F32):
    return OPS.fft_pass_info(c.kind, list(c.shape), c.axis, c.n, tin == BF16, tout == BF16)


def _field(info, name):
    return int(re.search(rf"\b{name}=(\d+)", info).group(1))


def _matches(expect, info):
    return expect.search(info) is not None if isinstance(expect, re.Pattern) else expect in info


def _configs():
    out = []
    for entry in OPS.fft_fixed_configs().strip(";").split(";"):
        L, cols, TP, T, rad = entry.split()
        out.append((int(L), int(cols), int(TP), int(T), rad))
    return out


def _largest_prime_at_most(n):
    while any(n % f == 0 for f in range(2, int(n ** 0.5) + 1)):
        n -= 1
    return n


# ------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_case_dispatch(case):
    for tin, tout in case.dtypes:
        info = _info(case, tin, tout)
        assert _matches(case.expect, info), (case.expect, info)


def test_fixed_configs_hit_or_dead():
    cfgs = _configs()
    assert len(cfgs) == 19
    default = {}
    for L, _, _, _, rad in cfgs:
        default.setdefault(L, rad)
    tuning = {c for c in cfgs if c[4] != default[c[0]]}
    assert tuning == TUNING_ONLY
    hit = set()
    for c in CASES:
        info = _info(c)
        if info.startswith("fixed"):
            hit.add(cfgs[_field(info, "cfg")][:4])
    shipped = {c[:4] for c in cfgs if c not in tuning}
    assert not hit & set(UNREACHABLE)
    missing = shipped - hit - set(UNREACHABLE)
    assert not missing, f"fixed configurations neither hit by CASES nor listed UNREACHABLE: {sorted(missing)}"
    assert set(UNREACHABLE) <= shipped


def test_unreachable_configs_never_win():
    """Brute force over the selection score: O in 1..64, I in 1..2048, all three kinds."""
    cfgs = _configs()
    for kind in ("r2c", "c2r", "c2c"):
        for L, cols in sorted({(k[0], k[1]) for k in UNREACHABLE}):
            wins = list(OPS.fft_fixed_sweep(kind, L, bool(cols), 2048, 64))
            assert sum(wins) == 2048 * 64
            for i, w in enumerate(wins):
                key = cfgs[i][:4]
                if key in UNREACHABLE:
                    assert w == 0, (kind, key, w)
                elif key[:2] == (L, cols) and cfgs[i] not in TUNING_ONLY:
                    assert w > 0, (kind, key)


def test_generic_tile_coverage():
    logt = {0: set(), 1: set()}
    ragged, odd_ragged = set(), set()
    for c in CASES:
        info = _info(c)
        if not info.startswith("generic"):
            continue
        T = 1 << _field(info, "logT")
        logt[_field(info, "cols")].add(_field(info, "logT"))
        if T > 1 and _field(info, "nsig") % T:
            ragged.add(c.kind)
            # an odd count: the unpaired signal is the last one, in the ragged last tile
            if c.kind != "c2c" and _field(info, "I") % 2:
                odd_ragged.add(c.kind)
    assert GENERIC_ROW_LOGT <= logt[0], logt
    assert GENERIC_COL_LOGT <= logt[1], logt
    assert ragged == {"r2c", "c2r", "c2c"}
    assert odd_ragged == {"r2c", "c2r"}


def test_headline_column_choices():
    """The H pass of rfft2 720x1440 runs over 721 spectral columns."""
    for batch, (TP, T) in {1: (90, 4), 2: (90, 8), 4: (45, 16)}.items():
        assert _fixed(720, 1, TP, T) in OPS.fft_pass_info("c2c", [batch, 720, 721], 1)
    assert _fixed(1440, 0, 288, 1) in OPS.fft_pass_info("r2c", [1, 720, 1440], 2)


def test_lds_limit_and_large_prime():
    assert OPS.fft_pass_info("r2c", [3, 6553], 1).startswith("large")
    assert OPS.fft_pass_info("r2c", [3, 6552], 1).startswith("generic L=6552 radices=[13,9,8,7] ")
    p = _largest_prime_at_most(6552)
    assert f"radices=[{p}] " in OPS.plan_info(p)
    assert OPS.fft_pass_info("c2c", [3, p], 1).startswith(f"generic L={p} radices=[{p}] ")


# ------------------------------------------------------------------ GPU tier
def _tol(n, tout):
    # fp32 out: the project's error model with its 2x margin; bf16 out: plus half a bf16 ulp
    return long_fft_tol(n) + (2.0 ** -9 if tout == BF16 else 0.0)


def _check(name, got, ref, dim, n, tout, pairs):
    tol = _tol(n, tout)
    err, worst = per_signal_rel_l2(got, ref, dim, pairs)
    glob = rel_l2(got, ref)
    print(f"{name}: per-signal {err:.3e} (signal {worst}) global {glob:.3e} bound {tol:.3e}")
    if tout == BF16 and err >= tol:  # near-zero outputs: against the fp64 result rounded to bf16
        err, worst = per_signal_rel_l2(got, ref.to(torch.bfloat16), dim, pairs)
        print(f"{name}: per-signal vs bf16-rounded reference {err:.3e} (signal {worst})")
    assert err < tol, f"{name}: signal {worst} off by {err:.3e} >= {tol:.3e}"
    assert glob < tol, f"{name}: global {glob:.3e} >= {tol:.3e}"


def _inputs(case, seed):
    """{input dtype: CPU input in that dtype}; the reference is computed from these same values."""
    shape = list(case.shape) + ([] if case.kind == "r2c" else [2])
    base = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return {tin: base.to(DT[tin]) for tin in sorted({t for t, _ in case.dtypes})}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_case_matches_fp64(device, case):
    n, ax = case.n, case.axis
    refs = {}
    for tin, x in _inputs(case, 1234).items():
        xd = x.double()
        if case.kind == "r2c":
            refs[tin] = (torch.view_as_real(torch.fft.rfft(xd, dim=ax)),)
        elif case.kind == "c2r":
            refs[tin] = (torch.fft.irfft(torch.view_as_complex(xd), n=n, dim=ax),)
        else:
            z = torch.view_as_complex(xd)
            refs[tin] = (torch.view_as_real(torch.fft.fft(z, dim=ax)), torch.view_as_real(torch.fft.ifft(z, dim=ax)))
        refs[tin] = (x.to(device),) + refs[tin]
    for tin, tout in case.dtypes:
        x, *ref = refs[tin]
        name = f"{_case_id(case)} {tin}->{tout}"
        if case.kind == "r2c":
            y = tdp.rfft(x, dim=ax, return_real=True, out_dtype=DT[tout])
            assert y.dtype == DT[tout] and y.shape == ref[0].shape
            _check(name, y, ref[0], ax, n, tout, True)
        elif case.kind == "c2r":
            y = tdp.irfft(x, n=n, dim=ax, out_dtype=DT[tout])
            assert y.dtype == DT[tout] and y.shape == ref[0].shape
            _check(name, y, ref[0], ax, n, tout, False)
        else:
            y = OPS.c2c(x, [ax], False, 1.0, DT[tout])
            assert y.dtype == DT[tout]
            _check(name + " forward", y, ref[0], ax, n, tout, True)
            y = OPS.c2c(x, [ax], True, 1.0 / n, DT[tout])
            _check(name + " inverse", y, ref[1], ax, n, tout, True)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,n,win", [
    ((40, 20, 27), 143, (12, 8, 30, 25)),  # generic columns, T = 8, ragged
    ((9, 31, 305), 720, (20, 11, 100, 64)),  # 720 columns (45, 16)
], ids=["generic143", "fixed720"])
def test_pruned_windows(device, shape, n, win):
    """c2c_axis with in_lo + in_hi < n and out_lo + out_hi < n: the stored_index gather and the
    pruned instantiations, forward and inverse."""
    in_lo, in_hi, out_lo, out_hi = win
    assert shape[1] == in_lo + in_hi
    full_shape = [shape[0], n, shape[2]]
    info = OPS.fft_pass_info("c2c", full_shape, 1)
    assert ("logT=3" in info) if n == 143 else (_fixed(720, 1, 45, 16) in info), info
    x = torch.randn(*shape, 2, generator=torch.Generator().manual_seed(7))
    z = torch.view_as_complex(x.double())
    full = torch.zeros(full_shape, dtype=torch.complex128)
    full[:, :in_lo] = z[:, :in_lo]
    full[:, n - in_hi:] = z[:, in_lo:]
    xd = x.to(device)
    for inverse in (False, True):
        r = torch.fft.ifft(full, dim=1, norm="forward") if inverse else torch.fft.fft(full, dim=1)
        ref = torch.view_as_real(torch.cat([r[:, :out_lo], r[:, n - out_hi:]], 1))
        y = OPS.c2c_axis(xd, 1, n, in_lo, in_hi, out_lo, out_hi, inverse, 1.0)
        assert y.shape == ref.shape
        _check(f"pruned n={n} inverse={inverse}", y, ref, 1, n, F32, True)


ADD_LAYOUTS = {
    "row143": ((5, 72), 1, 143, "generic L=143"),  # 5 signals: the last unpaired
    "col143": ((3, 72, 7), 1, 143, "generic L=143"),
    "col143T8": ((40, 72, 53), 1, 143, "logT=3"),
    "row512": ((3, 257), 1, 512, _fixed(512, 0, 64, 2)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("nadd", [1, 2])
@pytest.mark.parametrize("layout", list(ADD_LAYOUTS))
def test_c2r_add(device, layout, nadd, dt):
    """Addends fused into the C2R store: the generic kernel's add1 / add2 loads and the row-like
    fixed NADD variants, fp32 and bf16, odd signal counts."""
    shape, ax, n, expect = ADD_LAYOUTS[layout]
    assert expect in OPS.fft_pass_info("c2r", list(shape), ax, n)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(*shape, 2, generator=g).to(DT[dt])
    oshape = list(shape)
    oshape[ax] = n
    adds = [torch.randn(oshape, generator=g).to(DT[dt]) for _ in range(nadd)]
    ref = 0.5 * torch.fft.irfft(torch.view_as_complex(x.double()), n=n, dim=ax, norm="forward")
    for a in adds:
        ref = ref + a.double()
    dev = [a.to(device) for a in adds] + [None] * (2 - nadd)
    y = OPS.c2r_add(x.to(device), [ax], [n], 0.5, [], dev[0], dev[1], DT[dt])
    assert y.dtype == DT[dt] and list(y.shape) == oshape
    _check(f"c2r_add {layout} nadd={nadd} {dt}", y, ref, ax, n, dt, False)


@pytest.mark.gpu
def test_c2r_add_rejects_bad_addends(device):
    x = torch.randn(4, 72, 2, device=device)
    good = torch.randn(4, 143, device=device)
    OPS.c2r_add(x, [1], [143], 1.0, [], good, None, None)
    msg = "addend must be contiguous with the output's shape, dtype and device"
    with pytest.raises(RuntimeError, match=msg):
        OPS.c2r_add(x, [1], [143], 1.0, [], good.to(torch.bfloat16), None, None)
    with pytest.raises(RuntimeError, match=msg):
        OPS.c2r_add(x, [1], [143], 1.0, [], None, torch.randn(143, 4, device=device).t(), None)


# 11 * 11, 13 * 11, 13 * 13, 16 * 11, 15 * 15, 17 * 17, 23 * 19, 15 * 11 * 7 * 2, 17^3, the LDS limit
# (13 * 9 * 8 * 7) and the largest prime below it: radices 11, 13, 15 and generic primes in passes that
# have twiddles and a root table at a non-zero offset
LENGTHS = [121, 143, 169, 176, 225, 289, 437, 2310, 4913, 6552, _largest_prime_at_most(6552)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_multi_pass_lengths(device, n):
    g = torch.Generator().manual_seed(n)
    if n == LENGTHS[-1]:
        # The single-pass prime runs its direct n-point DFT on one thread per signal (L / R = 1
        # butterfly): 3.6 s per launch on MI355X whatever the batch (14.4 s measured for the four
        # transforms at batch 3).  One launch: the forward C2C at batch 1.
        z = torch.randn(1, n, 2, generator=g)
        ref = torch.view_as_real(torch.fft.fft(torch.view_as_complex(z.double()), dim=1))
        _check(f"fft {n}", OPS.c2c(z.to(device), [1], False, 1.0, None), ref, 1, n, F32, True)
        return
    x = torch.randn(3, n, generator=g)
    z = torch.randn(3, n, 2, generator=g)
    X = torch.fft.rfft(x.double(), dim=1)
    zc = torch.view_as_complex(z.double())
    _check(f"rfft {n}", tdp.rfft(x.to(device), return_real=True), torch.view_as_real(X), 1, n, F32, True)
    h = torch.randn(3, n // 2 + 1, 2, generator=g)
    _check(f"irfft {n}", tdp.irfft(h.to(device), n=n), torch.fft.irfft(torch.view_as_complex(h.double()), n=n, dim=1),
           1, n, F32, False)
    _check(f"fft {n}", OPS.c2c(z.to(device), [1], False, 1.0, None), torch.view_as_real(torch.fft.fft(zc, dim=1)),
           1, n, F32, True)
    _check(f"ifft {n}", OPS.c2c(z.to(device), [1], True, 1.0 / n, None), torch.view_as_real(torch.fft.ifft(zc, dim=1)),
           1, n, F32, True)


def _offset_view(shape, dtype, device, seed):
    """A contiguous view one element into a larger buffer, and an aligned copy of the same values."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.randn(numel + 1, generator=torch.Generator().manual_seed(seed)).to(dtype).to(device)
    v = buf[1:].view(shape)
    assert v.is_contiguous() and v.storage_offset() == 1
    assert v.data_ptr() % (2 * v.element_size()) != 0
    a = v.clone()
    assert a.data_ptr() % 16 == 0
    return v, a


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("shape", [(16, 48, 34), (4, 720), (2, 90, 24)], ids=["generic", "fixedrow", "fixedcol"])
def test_unaligned_real_input(device, shape, dt):
    """The real side's vector loads are guarded by pointer tests: same bits as the aligned call."""
    v, a = _offset_view(shape, DT[dt], device, 5)
    for odt in (torch.float32, DT[dt]):
        assert torch.equal(OPS.r2c(v, [1], 1.0, [], odt), OPS.r2c(a, [1], 1.0, [], odt))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("shape", [(16, 48, 34), (4, 720), (2, 90, 24)], ids=["generic", "fixedrow", "fixedcol"])
def test_unaligned_complex_input(device, shape, dt):
    """A complex input whose pointer is not aligned to one (re, im) pair is copied by the entry
    points (the kernels load whole pairs): same bits as the aligned call."""
    v, a = _offset_view(tuple(shape) + (2,), DT[dt], device, 6)
    n = shape[1]
    assert torch.equal(OPS.c2c(v, [1], False, 1.0, None), OPS.c2c(a, [1], False, 1.0, None))
    assert torch.equal(OPS.c2c(v, [1], True, 1.0, torch.float32), OPS.c2c(a, [1], True, 1.0, torch.float32))
    # n stored modes of an n-point C2R: those past the half spectrum are ignored (irfft semantics)
    assert torch.equal(OPS.c2r(v, [1], [n], 1.0, [], None), OPS.c2r(a, [1], [n], 1.0, [], None))
    add = torch.randn(shape, device=device).to(DT[dt])
    assert torch.equal(OPS.c2r_add(v, [1], [n], 1.0, [], add, None, None), OPS.c2r_add(a, [1], [n], 1.0, [], add, None, None))
    assert torch.equal(OPS.c2c_axis(v, 1, n, n - 3, 3, 5, 4, True, 1.0), OPS.c2c_axis(a, 1, n, n - 3, 3, 5, 4, True, 1.0))
