"""What the hand MFMA spectral kernels promise about memory they must not touch, on the GPU
(csrc/spectral/{legendre, sfno_mix, fno_pointwise_mfma, fno_c2r_pw_wide, afno_mlp}.hip):

1. Guard bands -- "nothing is loaded or stored outside x, the padded table or y".  Every device tensor the kernel
   touches (inputs, pre-split tables / weights, bias, spec and, through the ``_out`` ops, the output) is a view
   inside a larger buffer with ``GUARD`` elements of one fixed NaN bit pattern on each side.  After a normal run the
   output is finite and within the op's own bound, and every guard and every input is bitwise unchanged (compared as
   integers: a NaN overwritten by another NaN fails).
2. Poison -- "the part ``tri`` declares zero is not read".  NaN / Inf in x[q < m] (``legendre``, ``tri = 2``) and in
   c[l < m] (``sfno_mix``, ``tri = 1``) must not reach the result (the CPU tier of the same contract:
   tests/test_sht.py, tests/test_sfno_mix.py).
3. Stale LDS -- "edges are WRITTEN as zeros into the slab image (0 * stale-NaN is NaN)".  ``lds_poison()`` fills
   every CU's LDS with NaNs; the kernel launched right after it on the same stream must still give a finite, correct
   result at shapes that exercise every documented zero-fill.

Not covered: the spectral-only instances of fno_c2r_pw_wide.hip (``fno_c2r``, cin = 0), which have no ``_out`` op.

The tests only inspect buffers after normal runs; nothing is provoked.  References, cases and bounds are those of the
ops' own test files (fp64 references built once and shared through their caches): 1e-5 per field for ``legendre``,
``sfno_mix`` and split-weight ``afno_mlp``; per output channel 2e-5 (fp32 I/O) and 1e-2 (bf16 I/O) for the two FNO
ops, whose fp32 error carries the spec / GELU epilogue besides the bf16x3 product (measured up to 1.4e-5)."""
import re

import pytest
import torch

import test_afno_mlp as MLP
import test_fno_channels as PW
import test_fno_tail_wide as TAIL
import test_sfno_mix_gpu as MIX
import test_sht_gpu as LEG
from helpers import rel_l2
from tensorrt_dft_plugins_amd.ops import spectral as SP
from tensorrt_dft_plugins_amd.ops.sht import legendre_split

ops = torch.ops.amd_dft
GUARD = 4096
TOL = 1e-5  # legendre, sfno_mix (tests/test_sht_gpu.py, tests/test_sfno_mix_gpu.py); the FNO ops: PW.TOL, TAIL.TOL


def _fields(info):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", info)}


class Guarded:
    """A contiguous device tensor as a view inside a buffer with GUARD elements of a fixed NaN bit pattern (its own:
    ``tag`` lands in the mantissa) on each side, ``offset`` more in front.  ``t = None``: an output, pattern inside
    too, so an element the kernel did not write stays NaN."""

    def __init__(self, device, tag, t=None, shape=None, dtype=None, offset=0):
        shape, dtype = (t.shape, t.dtype) if t is not None else (shape, dtype)
        assert dtype in (torch.float32, torch.bfloat16)
        self.idt = torch.int32 if dtype == torch.float32 else torch.int16
        self.pattern = (0x7FC0_0000 | (0x1234 + tag)) if dtype == torch.float32 else (0x7FC0 | (1 + tag))
        n = 1
        for d in shape:
            n *= d
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.bits = torch.full((self.hi + GUARD,), self.pattern, dtype=self.idt, device=device)
        self.view = self.bits.view(dtype)[self.lo:self.hi].view(shape)
        self.src = None
        if t is not None:
            self.view.copy_(t)
            self.src = t.contiguous().view(self.idt).flatten()
        assert self.view.is_contiguous()

    def guards_intact(self):
        b = self.bits.cpu()
        return bool((b[:self.lo] == self.pattern).all()) and bool((b[self.hi:] == self.pattern).all())

    def unchanged(self):
        return torch.equal(self.bits[self.lo:self.hi].cpu(), self.src)


def _check_untouched(inputs, out):
    torch.cuda.synchronize()
    for i, g in enumerate(inputs):
        assert g.guards_intact(), f"guard of input {i} changed"
        assert g.unchanged(), f"input {i} changed"
    assert out.guards_intact(), "guard of the output changed"
    assert torch.isfinite(out.view.float()).all()


# ------------------------------------------------------------------------------------------------ legendre
# (N, Q, R, M) -> (MT, CT): one shape per kernel instance, ragged in every tiled dimension (Q % 32, R % 16 with a
# short last row group, M % MT, N % (8 CT)).  The first and last are cases of tests/test_sht_gpu.py; its own
# (4, 2) and (8, 2) cases have N and M on tile boundaries, so these two are the same grids (256 workgroups) with
# N = 17 and M = 127 / 252.
LEG_CASES = {(3, 45, 23, 13): (4, 1), (17, 33, 200, 127): (4, 2), (17, 33, 200, 252): (8, 2),
             (7, 33, 500, 252): (8, 1)}


def _leg_route(case, tri):
    N, Q, R, M = case
    f = _fields(ops.legendre_info(Q, R, M, 2 * N, tri))
    assert (f["MT"], f["CT"]) == LEG_CASES[case], f
    assert Q % 32 and R % 16 and M % f["MT"] and N % (8 * f["CT"])


def _leg_tensors(device, case, tri, x=None):
    N, Q, R, M = case
    x0, table, refs = LEG._case(case)
    t = LEG._zeroed(table, tri)
    gx = Guarded(device, 0, x0 if x is None else x)
    gt = Guarded(device, 1, t)
    gs = Guarded(device, 2, legendre_split(t))
    gy = Guarded(device, 3, shape=(N, R, M, 2), dtype=torch.float32)
    return gx, gt, gs, gy, refs[tri]


@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case", list(LEG_CASES), ids=lambda c: "x".join(map(str, c)))
def test_legendre_guard_bands(device, case, tri):
    _leg_route(case, tri)
    gx, gt, gs, gy, ref = _leg_tensors(device, case, tri)
    assert ops.legendre_out(gx.view, gt.view, gs.view, tri, gy.view) is gy.view
    _check_untouched([gx, gt, gs], gy)
    err = LEG._field_err(gy.view, ref, 1)
    print(f"MEASURED legendre guarded {case} tri={tri} {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("case", LEG.CASES[:2], ids=lambda c: "x".join(map(str, c)))
def test_legendre_poison_where_tri2_declares_zero(device, case, poison):
    """x[n, q < m, m] = NaN / Inf under ``tri = 2``: the result is the product of x with that part zero -- which is
    the product of the table with that part zero, the shared reference -- and finite."""
    N, Q, R, M = case
    x, table, refs = LEG._case(case)
    below = (torch.arange(Q)[:, None] < torch.arange(M)[None, :])[None, :, :, None].expand(N, Q, M, 2)
    xp = torch.where(below, poison, x).to(device)
    t = LEG._zeroed(table, 2).to(device)
    out = ops.legendre(xp, t, legendre_split(t), 2)
    assert torch.isfinite(out).all()
    err = LEG._field_err(out, refs[2], 1)
    print(f"MEASURED legendre poison {case} {poison} {err:.3e}")
    assert err < TOL


# ------------------------------------------------------------------------------------------------ sfno_mix
# cases of tests/test_sfno_mix_gpu.py (one tiling; what each must reach is its SHAPE table): one ragged slab and
# Cout < 16 | two slabs, ragged second row tile, batch-packed ragged column tile | two row groups, M > L | six
# column tiles per degree
MIX_CASES = [MIX.CASES[0], MIX.CASES[1], MIX.CASES[3], MIX.CASES[4]]


def _mix_route(case):
    f = _fields(ops.sfno_mix_info(*case, 0))
    assert (f["slabs"], f["otiles"], f["ogroups"], f["ctiles"]) == MIX.SHAPE[case] and f["coltile"] == 64


def _mix_tensors(device, case, tri):
    B, Cin, Cout, L, M = case
    c, w, refs = MIX._case(case)
    gc = Guarded(device, 0, c * MIX._keep(L, M) if tri else c)
    gw = Guarded(device, 1, w)
    gs = Guarded(device, 2, SP.sfno_mix_split(w))
    gy = Guarded(device, 3, shape=(B, Cout, L, M, 2), dtype=torch.float32)
    return gc, gw, gs, gy, refs[tri]


@pytest.mark.gpu
@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("case", MIX_CASES, ids=lambda c: "x".join(map(str, c)))
def test_sfno_mix_guard_bands(device, case, tri):
    _mix_route(case)
    gc, gw, gs, gy, ref = _mix_tensors(device, case, tri)
    assert ops.sfno_mix_out(gc.view, gw.view, gs.view, tri, gy.view) is gy.view
    _check_untouched([gc, gw, gs], gy)
    err = MIX._field_err(gy.view, ref)
    print(f"MEASURED sfno_mix guarded {case} tri={tri} {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("case", MIX.CASES[:2], ids=lambda c: "x".join(map(str, c)))
def test_sfno_mix_poison_where_l_below_m(device, case, poison):
    """c[b, i, l, m > l] = NaN / Inf under ``tri = 1``: the product of the zeroed spectrum, exact 0.0 where l < m."""
    B, Cin, Cout, L, M = case
    c, w, refs = MIX._case(case)
    keep = MIX._keep(L, M)
    cp = torch.where(keep[None, None].expand(B, Cin, L, M, 2), c, poison).to(device)
    wd = w.to(device)
    out = ops.sfno_mix(cp, wd, SP.sfno_mix_split(wd), 1)
    assert torch.isfinite(out).all()
    err = MIX._field_err(out, refs[1])
    print(f"MEASURED sfno_mix poison {case} {poison} {err:.3e}")
    assert err < TOL
    assert torch.all(out.cpu()[(~keep)[None, None].expand(B, Cout, L, M, 2)] == 0.0)


# ------------------------------------------------------------------------------------------------ fno_pointwise
# (case of tests/test_fno_channels.py, offset of x / spec / y in their storage) -> per-element I/O?  Aligned with
# P % 4 == 0 (Cin % 32, Cout % 16, P % 256 ragged) | the same one element into the storage | odd P with one live row
# in the second slab and one live column in the second tile | odd P, three slabs, two output groups (that file's
# 96 -> 65 case with Cin = 72, so that the last slab is ragged here too)
PW_CASES = [((2, 40, 40, 16, 24), 0, 4), ((2, 40, 40, 16, 24), 1, 1), ((1, 33, 17, 9, 7), 0, 1),
            ((1, 72, 65, 3, 21), 0, 1)]
# spec / bias / GELU: each on and off (GELU picks the kernel instance)
PW_FLAGS = [(True, True, True), (False, False, False), (True, False, False), (False, True, True)]


def _pw_run(device, case, dt, offset, flags, before=None):
    """One guarded fno_pointwise_out run -> (guarded inputs, guarded output, error against the fp64 reference)."""
    B, Ci, Co, H, W = case
    use_spec, use_bias, gelu = flags
    x, s, w, b = PW._inputs(case, dt, 31)
    gx = Guarded(device, 0, x, offset=offset)
    gs = Guarded(device, 1, s, offset=offset)
    gw, gb = Guarded(device, 2, w), Guarded(device, 3, b)
    gy = Guarded(device, 4, shape=(B, Co, H, W), dtype=dt, offset=offset)
    args = (gs.view if use_spec else None, gx.view, gw.view, gb.view if use_bias else None, gelu, gy.view)
    if before is not None:
        before(lambda: ops.fno_pointwise_out(*args))
    assert ops.fno_pointwise_out(*args) is gy.view
    ref = PW._reference(x, w, s if use_spec else None, b if use_bias else None, gelu)
    return [gx, gs, gw, gb], gy, ref


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case,offset,vp", PW_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fno_pointwise_mfma_guard_bands(device, case, offset, vp, dt):
    """The MFMA kernel's instances: fp32 (x3) / bf16 I/O (asserted through the info string) x vector / per-element
    I/O (forced by alignment and P, not reported by the info string) x GELU on / off."""
    B, Ci, Co, H, W = case
    f = _fields(ops.fno_pointwise_info(Ci, Co, dt == torch.bfloat16, H * W))
    assert ops.fno_pointwise_info(Ci, Co, dt == torch.bfloat16, H * W).startswith("mfma ")
    assert f["x3"] == (dt == torch.float32) and f["vp"] == (4 if (H * W) % 4 == 0 else 1)
    assert Ci % 32 and Co % 16 and (H * W) % 256
    for flags in PW_FLAGS:
        inputs, gy, ref = _pw_run(device, case, dt, offset, flags)
        # the test's own setup, not the kernel's path: fno_pointwise_info describes aligned tensors only.  The launch
        # takes per-element I/O when x, y or spec start off a 4-element boundary or P % 4 != 0, which is what the
        # offset-1 and odd-P cases arrange
        assert (gy.view.data_ptr() % (4 * gy.view.element_size()) == 0 and (H * W) % 4 == 0) == (vp == 4)
        _check_untouched(inputs, gy)
        err = PW._chan_err(gy.view.float(), ref)
        print(f"MEASURED fno_pointwise guarded {case} off={offset} {dt} spec/bias/gelu={flags} {err:.3e}")
        assert err < PW.TOL[dt]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fno_pointwise_fixed_guard_bands(device, dt):
    """The op's other route, a register-resident instance (Cin = 20), with vector and per-element I/O."""
    for case in ((2, 20, 24, 6, 10), (1, 20, 24, 5, 13)):
        assert ops.fno_pointwise_info(case[1], case[2], dt == torch.bfloat16, case[3] * case[4]).startswith("fixed ")
        for flags in PW_FLAGS[:2]:
            inputs, gy, ref = _pw_run(device, case, dt, 0, flags)
            _check_untouched(inputs, gy)
            err = PW._chan_err(gy.view.float(), ref)
            print(f"MEASURED fno_pointwise fixed guarded {case} {dt} spec/bias/gelu={flags} {err:.3e}")
            assert err < PW.TOL[dt]


# ------------------------------------------------------------------------------------------------ fno_c2r_pw
# (B, Cin, Cout, H, W, m) -> weights in LDS?  The first is a case of tests/test_fno_tail_wide.py (last slab and last
# group ragged, chunks 64 * 3 + 8, m % 16 != 0); the second is its 521-channel case (weights beyond LDS in both
# dtypes, per-element weight loads) at W = 72, m = 5, so that the last chunk and the mode slab are ragged there too.
TAIL_CASES = {(2, 33, 65, 3, 200, 20): 1, (1, 521, 65, 2, 72, 5): 0}
TAIL_FLAGS = [(True, True), (False, False)]  # (gelu, bias): GELU picks the kernel instance


def _tail_run(device, shape, dt, flags, before=None):
    B, Ci, Co, H, W, m = shape
    gelu, bias = flags
    yw, x, wc, b, ref = TAIL._inputs(shape + flags, dt)
    gyw, gx, gw = Guarded(device, 0, yw), Guarded(device, 1, x), Guarded(device, 2, wc)
    inputs = [gyw, gx, gw]
    if bias:
        inputs.append(Guarded(device, 3, b))
    gy = Guarded(device, 4, shape=(B, Co, H, W), dtype=dt)
    args = (gyw.view, gx.view, gw.view, inputs[3].view if bias else None, gelu, gy.view)
    if before is not None:
        before(lambda: ops.fno_c2r_pw_out(*args))
    assert ops.fno_c2r_pw_out(*args) is gy.view
    return inputs, gy, ref


@pytest.mark.gpu
@pytest.mark.parametrize("flags", TAIL_FLAGS, ids=["gelu-bias", "plain"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", list(TAIL_CASES), ids=lambda s: "x".join(map(str, s)))
def test_fno_c2r_pw_wide_guard_bands(device, shape, dt, flags):
    """The wide kernel's instances: fp32 (x3) / bf16 I/O x GELU on / off x weights in LDS / from global memory."""
    B, Ci, Co, H, W, m = shape
    info = ops.fno_c2r_pw_info(Ci, Co, m, W, dt == torch.bfloat16)
    f = _fields(info)
    assert info.startswith("wide ") and f["x3"] == (dt == torch.float32) and f["wl"] == TAIL_CASES[shape], info
    assert Ci % 32 and Co % 16 and W % 64 and m % 16
    inputs, gy, ref = _tail_run(device, shape, dt, flags)
    _check_untouched(inputs, gy)
    err = TAIL._chan_err(gy.view.float(), ref)
    print(f"MEASURED fno_c2r_pw wide guarded {shape} {dt} gelu/bias={flags} {err:.3e}")
    assert err < TAIL.TOL[dt]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,route", [((2, 7, 13, 3, 200, 20), "fused"), ((1, 40, 48, 2, 100, 20), "split")],
                         ids=["fused", "split"])
def test_fno_c2r_pw_other_routes_guard_bands(device, shape, route, dt):
    """The op's other two routes: the narrow fused kernel, and C2R + the pointwise kernel writing into ``out``."""
    B, Ci, Co, H, W, m = shape
    assert ops.fno_c2r_pw_info(Ci, Co, m, W, dt == torch.bfloat16).startswith(route)
    inputs, gy, ref = _tail_run(device, shape, dt, (True, True))
    _check_untouched(inputs, gy)
    err = TAIL._chan_err(gy.view.float(), ref)
    print(f"MEASURED fno_c2r_pw {route} guarded {shape} {dt} {err:.3e}")
    assert err < TAIL.TOL[dt]  # the bounds of tests/test_fno.py and tests/test_fno_tail_wide.py for these routes


@pytest.mark.gpu
def test_out_variants_refuse_what_they_cannot_write_gpu(device):
    """On the device too: a wrong shape, a non-contiguous view and a start off the kernel's store boundary raise."""
    x, table, _ = LEG._case(LEG.CASES[0])
    N, Q, R, M = LEG.CASES[0]
    xd, td = x.to(device), table.to(device)
    buf = torch.empty(N * R * M * 2 + 1, device=device)
    for bad in (torch.empty(N, R, M + 1, 2, device=device), torch.empty(N, R, M, 4, device=device)[..., ::2],
                buf[1:].view(N, R, M, 2), torch.empty(N, R, M, 2)):
        with pytest.raises(RuntimeError, match="out must"):
            ops.legendre_out(xd, td, None, 0, bad)
    c, w, _ = MIX._case(MIX.CASES[0])
    B, Cin, Cout, L, Mo = MIX.CASES[0]
    buf = torch.empty(B * Cout * L * Mo * 2 + 1, device=device)
    for bad in (torch.empty(B, Cout, L, Mo, 4, device=device)[..., ::2], buf[1:].view(B, Cout, L, Mo, 2)):
        with pytest.raises(RuntimeError, match="out must"):
            ops.sfno_mix_out(c.to(device), w.to(device), None, 0, bad)
    yw, xt, wc, b, _ = TAIL._inputs(TAIL.CASES[2], torch.float32)
    Bt, Ci, Co, H, W = 1, 7, 40, 2, 72
    buf = torch.empty(Bt * Co * H * W + 2, device=device)
    for bad in (torch.empty(Bt, Co, H, 2 * W, device=device)[..., ::2], buf[2:].view(Bt, Co, H, W)):
        with pytest.raises(RuntimeError, match="out must"):
            ops.fno_c2r_pw_out(yw.to(device), xt.to(device), wc.to(device), None, False, bad)


# ------------------------------------------------------------------------------------------------ afno_mlp
# (block size, split, tokens) -> token tile: every instance of the kernel (packing x 64 / 32 / 16 token rows), T = 65
# (a last tile of one row at 64 and 32, of one row in the fifth tile at 16); plain weights reach the 16-row tile only
# for a handful of tokens, so that instance runs T = 9 (seven zero rows)
MLP_CASES = {(32, False, 65): 64, (32, True, 65): 64, (160, False, 65): 32, (80, True, 65): 32, (256, True, 65): 16,
             (16, False, 9): 16}


def _mlp_route(bs, split, T):
    f = _fields(ops.afno_mlp_info(bs, split, T))
    assert f["TOK"] == MLP_CASES[(bs, split, T)] and f["x3"] == split and T % f["TOK"]


@pytest.mark.gpu
@pytest.mark.parametrize("bs,split,T", list(MLP_CASES), ids=lambda v: str(v))
def test_afno_mlp_guard_bands(device, bs, split, T):
    """Every instance with x, the packed weights, the biases and the output between guard bands (tests/test_afno_mlp.py
    guards x and y of the 64-row tile).  References and bounds of that file."""
    _mlp_route(bs, split, T)
    x, (w1, b1, w2, b2), nb, ref, ref_bf = MLP._case(bs, T)
    inputs = [Guarded(device, 0, x)]
    inputs += [Guarded(device, 1 + i, t) for i, t in enumerate(SP.pack_afno_weights(w1, b1, w2, b2, split))]
    gy = Guarded(device, 5, shape=x.shape, dtype=torch.float32)
    assert ops.afno_mlp_out(*(g.view for g in inputs), 0.01, gy.view) is gy.view
    _check_untouched(inputs, gy)
    err = rel_l2(gy.view, ref if split else ref_bf)
    print(f"MEASURED afno_mlp guarded bs={bs} split={split} T={T} {err:.3e}")
    assert err < (1e-5 if split else 6e-3)


# ------------------------------------------------------------------------------------------------ stale LDS
# These depend on stream order alone: lds_poison() and the kernel under test are consecutive launches on the current
# stream, everything the op needs is pre-split, contiguous and aligned, and a first call before the poison has
# already built whatever the op caches (the tail's DFT tables), so no other kernel runs in between.  A plain run is
# serial anyway.  The mark is pytest-xdist's and matters only under ``--dist loadgroup``, where it keeps these tests in
# one worker (another process's kernels in between would overwrite the poison and blind them); without xdist
# installed it is an unknown mark, reported as a warning -- registering it belongs to the pytest settings, which stay
# as they are.
lds = pytest.mark.xdist_group(name="stale_lds")


def _poison_then(run):
    run()  # caches (DFT tables, kernel attributes) are built before the poison, not between it and the kernel
    torch.cuda.synchronize()
    ops.lds_poison()


@pytest.mark.gpu
@lds
def test_lds_poison_survives_to_the_next_kernel(device):
    """The premise of this section: a kernel launched right after ``lds_poison()`` finds the NaN pattern in every
    LDS word it can reach.  A runtime that starts clearing LDS between kernels turns this red instead of leaving the
    tests below silently blind."""
    f = _fields(ops.lds_poison_info())
    print(f"MEASURED lds_poison geometry {f}")
    # a poison / probe workgroup holds a whole CU's LDS, 160 KiB: no smaller than the largest request of a kernel
    # under test (the wide tail's tables + weights), so no part of LDS those kernels can get is left unpoisoned
    assert f["bytes"] >= 160 * 1024 and f["wgs"] >= 4 * torch.cuda.get_device_properties(device).multi_processor_count
    for _ in range(3):
        ops.lds_poison()
        frac = float(ops.lds_probe())
        print(f"MEASURED lds_probe fraction {frac:.6f}")
        assert frac == 1.0


@pytest.mark.gpu
@lds
@pytest.mark.parametrize("tri", [0, 1, 2])
@pytest.mark.parametrize("case", list(LEG_CASES), ids=lambda c: "x".join(map(str, c)))
def test_legendre_stale_lds(device, case, tri):
    """q >= Q, n >= N and m >= M of the slab image must be written as zeros: Q % 32, N % NT, M % MT all non-zero."""
    _leg_route(case, tri)
    gx, gt, gs, gy, ref = _leg_tensors(device, case, tri)
    _poison_then(lambda: ops.legendre_out(gx.view, gt.view, gs.view, tri, gy.view))
    ops.legendre_out(gx.view, gt.view, gs.view, tri, gy.view)
    assert torch.isfinite(gy.view).all()
    err = LEG._field_err(gy.view, ref, 1)
    print(f"MEASURED legendre stale-lds {case} tri={tri} {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
@lds
@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("case", [MIX.CASES[1], MIX.CASES[4]], ids=lambda c: "x".join(map(str, c)))
def test_sfno_mix_stale_lds(device, case, tri):
    """i >= Cin and dead columns must be written as zeros: Cin % 16 != 0 with a ragged last column tile (20 -> 20, 26
    columns), and under ``tri = 1`` low degrees whose last tile leaves waves idle (five batch entries, 70 orders)."""
    B, Cin, Cout, L, M = case
    _mix_route(case)
    gc, gw, gs, gy, ref = _mix_tensors(device, case, tri)
    _poison_then(lambda: ops.sfno_mix_out(gc.view, gw.view, gs.view, tri, gy.view))
    ops.sfno_mix_out(gc.view, gw.view, gs.view, tri, gy.view)
    assert torch.isfinite(gy.view).all()
    err = MIX._field_err(gy.view, ref)
    print(f"MEASURED sfno_mix stale-lds {case} tri={tri} {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
@lds
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case,offset,vp", PW_CASES[:3], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fno_pointwise_mfma_stale_lds(device, case, offset, vp, dt):
    """Rows i >= Cin of the last slab and pixels >= P must be written as zeros: Cin % 32, P % 256, Cout % 16 non-zero,
    every instance (dtype x vector / per-element I/O x GELU)."""
    B, Ci, Co, H, W = case
    assert ops.fno_pointwise_info(Ci, Co, dt == torch.bfloat16, H * W).startswith("mfma ")
    assert Ci % 32 and Co % 16 and (H * W) % 256
    for flags in PW_FLAGS[:2]:
        _, gy, ref = _pw_run(device, case, dt, offset, flags, before=_poison_then)
        assert torch.isfinite(gy.view.float()).all()
        err = PW._chan_err(gy.view.float(), ref)
        print(f"MEASURED fno_pointwise stale-lds {case} off={offset} {dt} spec/bias/gelu={flags} {err:.3e}")
        assert err < PW.TOL[dt]


@pytest.mark.gpu
@lds
@pytest.mark.parametrize("flags", TAIL_FLAGS, ids=["gelu-bias", "plain"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", list(TAIL_CASES), ids=lambda s: "x".join(map(str, s)))
def test_fno_c2r_pw_wide_stale_lds(device, shape, dt, flags):
    """Rows >= Cin and pixels >= W of the x slab must be written as zeros: Cin % 32, W % 64, Cout % 16 and m % 16
    non-zero, every instance."""
    B, Ci, Co, H, W, m = shape
    info = ops.fno_c2r_pw_info(Ci, Co, m, W, dt == torch.bfloat16)
    assert info.startswith("wide ") and _fields(info)["wl"] == TAIL_CASES[shape], info
    assert Ci % 32 and Co % 16 and W % 64 and m % 16
    _, gy, ref = _tail_run(device, shape, dt, flags, before=_poison_then)
    assert torch.isfinite(gy.view.float()).all()
    err = TAIL._chan_err(gy.view.float(), ref)
    print(f"MEASURED fno_c2r_pw wide stale-lds {shape} {dt} gelu/bias={flags} {err:.3e}")
    assert err < TAIL.TOL[dt]


@pytest.mark.gpu
@lds
@pytest.mark.parametrize("bs,split,T", list(MLP_CASES), ids=lambda v: str(v))
def test_afno_mlp_stale_lds(device, bs, split, T):
    """Rows past T of the operand tile must be written as zeros.  References and bounds of tests/test_afno_mlp.py."""
    _mlp_route(bs, split, T)
    x, (w1, b1, w2, b2), nb, ref, ref_bf = MLP._case(bs, T)
    xd = x.to(device)
    packed = [t.to(device) for t in SP.pack_afno_weights(w1, b1, w2, b2, split)]
    out = torch.full_like(xd, float("nan"))
    _poison_then(lambda: ops.afno_mlp_out(xd, *packed, 0.01, out))
    ops.afno_mlp_out(xd, *packed, 0.01, out)
    assert torch.isfinite(out).all()
    err = rel_l2(out, ref if split else ref_bf)
    print(f"MEASURED afno_mlp stale-lds bs={bs} split={split} T={T} {err:.3e}")
    assert err < (1e-5 if split else 6e-3)
