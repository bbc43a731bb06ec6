"""``afno_mlp``: the AFNO block-diagonal complex MLP on an already-transformed spectrum (csrc/spectral/afno_mlp.hip),
the route every AFNO shape outside the fused filter's 12 instances takes on the GPU.

CPU tier: the ATen op against an fp64 restatement of ``afno2d_reference``'s MLP + softshrink, the Meta shape, the
``afno_mlp_info`` strings, the Python gate against the info op, and the CPU model unchanged by the route.
GPU tier: the kernel against the fp64 reference over block sizes x ragged token counts, an exact-weights layout
check, a guard-band bounds check, ``afno2d_amd`` / ``AFNONet`` at non-instance shapes under ``strict_mode``, hipGraph
capture and run-to-run determinism."""
import pytest
import torch
import torch.nn.functional as F

from tensorrt_dft_plugins_amd import utils
from tensorrt_dft_plugins_amd.models import AFNOConfig, AFNONet
from tensorrt_dft_plugins_amd.models.afno import afno2d_amd, afno2d_reference
from tensorrt_dft_plugins_amd.ops import spectral as S
from helpers import rel_l2


def _params(nb, bs, scale=0.05, seed=0):
    g = torch.Generator().manual_seed(seed)
    w1 = scale * torch.randn(2, nb, bs, bs, generator=g)
    w2 = scale * torch.randn(2, nb, bs, bs, generator=g)
    b1 = scale * torch.randn(2, nb, bs, generator=g)
    b2 = scale * torch.randn(2, nb, bs, generator=g)
    return w1, b1, w2, b2


def _bf16_exact(t):
    return t.to(torch.bfloat16).float()


def mlp_ref64(x, w1, b1, w2, b2, nb, lam):
    """afno2d_reference's two-layer complex block MLP + softshrink on a given spectrum x [..., C, 2], in fp64."""
    x = x.double()
    w1, b1, w2, b2 = (t.double() for t in (w1, b1, w2, b2))
    C = x.shape[-2]
    z = x.reshape(*x.shape[:-2], nb, C // nb, 2)
    xr, xi = z[..., 0], z[..., 1]
    e = lambda a, w: torch.einsum("...bi,bio->...bo", a, w)  # noqa: E731
    o1r = F.relu(e(xr, w1[0]) - e(xi, w1[1]) + b1[0])
    o1i = F.relu(e(xi, w1[0]) + e(xr, w1[1]) + b1[1])
    o2r = e(o1r, w2[0]) - e(o1i, w2[1]) + b2[0]
    o2i = e(o1i, w2[0]) + e(o1r, w2[1]) + b2[1]
    return F.softshrink(torch.stack([o2r, o2i], dim=-1), lambd=lam).reshape(x.shape)


# ------------------------------------------------------------------------------------------------ CPU tier
# (NB, BS, split): the split layout is 32-column groups over K = 2 BS, so it does not exist at BS = 40
# (pack_afno_weights(split=True) raises there); BS = 48 stands in as the second split shape.
@pytest.mark.parametrize("nb,bs,split", [(4, 16, False), (4, 16, True), (8, 40, False), (2, 48, True)])
def test_cpu_op_vs_fp64_reference(nb, bs, split):
    """bf16-exact weights: both packings then hold the weights exactly, and the fp32 ATen op differs from the fp64
    reference by fp32 rounding alone."""
    torch.manual_seed(nb * 100 + bs)
    w1, b1, w2, b2 = _params(nb, bs, seed=bs)
    w1, w2 = _bf16_exact(w1), _bf16_exact(w2)
    x = torch.randn(2, 5, 3, nb * bs, 2)
    out = torch.ops.amd_dft.afno_mlp(x, *S.pack_afno_weights(w1, b1, w2, b2, split), 0.01)
    assert out.shape == x.shape and out.dtype == torch.float32
    err = rel_l2(out, mlp_ref64(x, w1, b1, w2, b2, nb, 0.01))
    print(f"MEASURED afno_mlp cpu nb={nb} bs={bs} split={split} {err:.3e}")
    assert err < 1e-6


def test_cpu_split_packing_needs_32_column_groups():
    w1, b1, w2, b2 = _params(8, 40)
    with pytest.raises(RuntimeError):
        S.pack_afno_weights(w1, b1, w2, b2, split=True)


def test_cpu_out_variant_and_meta_shape():
    nb, bs = 4, 16
    w1, b1, w2, b2 = _params(nb, bs)
    packed = S.pack_afno_weights(w1, b1, w2, b2)
    x = torch.randn(3, 7, nb * bs, 2)
    ref = torch.ops.amd_dft.afno_mlp(x, *packed, 0.01)
    out = torch.full_like(x, float("nan"))
    torch.ops.amd_dft.afno_mlp_out(x, *packed, 0.01, out)
    assert torch.equal(out, ref)
    m = torch.ops.amd_dft.afno_mlp(x.to("meta"), *(t.to("meta") for t in packed), 0.01)
    assert m.device.type == "meta" and m.shape == x.shape and m.dtype == torch.float32


def test_info_strings():
    info = torch.ops.amd_dft.afno_mlp_info
    for bs in (16, 32, 80, 256):
        for split in (False, True):
            s = info(bs, split, 1000)
            assert s.startswith("mfma TOK="), (bs, split, s)
            tok = int(s.split()[1].split("=")[1])
            assert tok in (16, 32, 64) and f"ksteps={bs // 16}" in s and f"x3={int(split)}" in s
            lds = int([f for f in s.split() if f.startswith("lds=")][0][4:])
            assert lds == 2 * (2 if split else 1) * tok * (2 * bs + 8) * 2 and lds <= 80 * 1024
            assert f"tiles={(1000 + tok - 1) // tok}" in s
    for bs in (40, 8, 272):
        assert info(bs, False, 1000).startswith("none "), bs
        assert info(bs, True, 1000).startswith("none "), bs
    # the token tile shrinks at large block sizes (LDS) and for a handful of tokens
    assert "TOK=64" in info(96, False, 1000) and "TOK=32" in info(96, True, 1000) and "TOK=16" in info(256, True, 1000)
    assert "TOK=16" in info(32, False, 1) and "TOK=32" in info(32, False, 20)


def test_python_gate_matches_info_op():
    for bs in range(8, 289, 8):
        for split in (False, True):
            ok = torch.ops.amd_dft.afno_mlp_info(bs, split, 64).startswith("mfma")
            assert S.afno_mlp_block_size_ok(bs) == ok, (bs, split)
    assert not S.afno_mlp_available(torch.zeros(1, 4, 4, 64), 4)  # the route is GPU only


def _cpu_model_output():
    torch.manual_seed(21)
    cfg = AFNOConfig(img_size=(32, 64), in_chans=3, out_chans=3, embed_dim=64, depth=2, num_blocks=4)
    m = AFNONet(cfg, backend="amd").eval()
    x = torch.randn(1, 3, 32, 64)
    with torch.no_grad():
        return m(x), m.set_backend("torch")(x)


def test_cpu_model_unchanged_by_the_route(monkeypatch):
    """AFNONet(backend="amd") on CPU (embed 64, 4 blocks: block size 16, which the GPU route takes) never reaches
    the new route, and its output is bit-identical to a run with both gates forced shut -- with them shut the code
    executed is, line for line, the code from before the route existed."""
    def boom(*a, **k):
        raise AssertionError("the afno_mlp route ran on CPU")

    monkeypatch.setattr(S, "afno_spectral_mlp", boom)
    monkeypatch.setattr(S, "afno_block_mlp_hand", boom)
    y, ref = _cpu_model_output()
    assert rel_l2(y, ref) < 1e-5
    monkeypatch.setattr(S, "afno_mlp_available", lambda x, nb: False)
    monkeypatch.setattr(S, "_mlp_hand_ok", lambda blk, x: False)
    y0, _ = _cpu_model_output()
    assert torch.equal(y, y0)


# ------------------------------------------------------------------------------------------------ GPU tier
_REF_CACHE = {}


def _case(bs, T, nb=None):
    """(x, params, fp64 references) of one (block size, tokens) case, built once."""
    nb = nb or (8 if bs == 16 else 2)
    key = (bs, T, nb)
    if key not in _REF_CACHE:
        g = torch.Generator().manual_seed(bs * 1000 + T)
        x = torch.randn(1, T, 1, nb * bs, 2, generator=g)
        p = _params(nb, bs, seed=bs + T)
        w1, b1, w2, b2 = p
        _REF_CACHE[key] = (x, p, nb, mlp_ref64(x, w1, b1, w2, b2, nb, 0.01),
                           mlp_ref64(x, _bf16_exact(w1), b1, _bf16_exact(w2), b2, nb, 0.01))
    return _REF_CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("bs", [16, 32, 80, 112, 256])
def test_op_vs_fp64_reference(device, bs, T):
    """Split weights against the fp64 MLP of the fp32 weights (< 1e-5); plain bf16 weights against the fp64 MLP of the
    weights the op is given, i.e. the bf16 values the packed layout holds (< 6e-3: what remains is the kernel's own
    rounding of the spectrum and the hidden activation to bf16) -- the references and bounds of the fused filter's
    tests (tests/test_spectral_gpu.py)."""
    x, (w1, b1, w2, b2), nb, ref, ref_bf = _case(bs, T)
    xd = x.to(device)
    o3 = torch.ops.amd_dft.afno_mlp(xd, *(t.to(device) for t in S.pack_afno_weights(w1, b1, w2, b2, True)), 0.01)
    o1 = torch.ops.amd_dft.afno_mlp(xd, *(t.to(device) for t in S.pack_afno_weights(w1, b1, w2, b2, False)), 0.01)
    assert o3.shape == x.shape and o3.dtype == torch.float32 and o1.shape == x.shape
    e3, e1 = rel_l2(o3, ref), rel_l2(o1, ref_bf)
    print(f"MEASURED afno_mlp bs={bs} T={T} split {e3:.3e} bf16 {e1:.3e}")
    assert e3 < 1e-5
    assert e1 < 6e-3


@pytest.mark.gpu
@pytest.mark.parametrize("bs,nb", [(16, 8), (80, 2)])
def test_layout_exact_weights(device, bs, nb):
    """Identity w1, 0.5 I + one asymmetric imaginary coupling in w2, one bias entry, integer spectra, lambda 0: every
    value is exact in bf16, so both packings must reproduce the reference to fp32 rounding (a transposed tile, a
    swapped re / im column or a wrong block would not)."""
    g = torch.Generator().manual_seed(bs)
    w1 = torch.zeros(2, nb, bs, bs)
    w1[0] = torch.eye(bs)
    w2 = torch.zeros(2, nb, bs, bs)
    w2[0] = torch.eye(bs) * 0.5
    w2[1, :, 0, 1] = 0.25
    b1 = torch.zeros(2, nb, bs)
    b2 = torch.zeros(2, nb, bs)
    b2[0, :, 3] = 1.0
    x = torch.randint(-3, 4, (1, 70, 1, nb * bs, 2), generator=g).float()
    ref = mlp_ref64(x, w1, b1, w2, b2, nb, 0.0)
    for split in (False, True):
        packed = [t.to(device) for t in S.pack_afno_weights(w1, b1, w2, b2, split)]
        err = rel_l2(torch.ops.amd_dft.afno_mlp(x.to(device), *packed, 0.0), ref)
        print(f"MEASURED afno_mlp exact bs={bs} split={split} {err:.3e}")
        assert err < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("split", [False, True])
def test_bounds_guard_bands(device, split):
    """x and the output are views inside larger NaN-filled buffers, T = 65 (a ragged second tile): the output is
    finite and correct and every guard element is still NaN.  The test only inspects; nothing is provoked."""
    bs, T = 32, 65
    x, (w1, b1, w2, b2), nb, ref, ref_bf = _case(bs, T)
    n, guard = x.numel(), 4096
    xbuf = torch.full((n + 2 * guard,), float("nan"), device=device)
    ybuf = torch.full((n + 2 * guard,), float("nan"), device=device)
    xv = xbuf[guard:guard + n].view(x.shape)
    xv.copy_(x)
    yv = ybuf[guard:guard + n].view(x.shape)
    packed = [t.to(device) for t in S.pack_afno_weights(w1, b1, w2, b2, split)]
    torch.ops.amd_dft.afno_mlp_out(xv, *packed, 0.01, yv)
    torch.cuda.synchronize()
    assert torch.isfinite(yv).all()
    assert rel_l2(yv, ref if split else ref_bf) < (1e-5 if split else 6e-3)
    for buf in (xbuf, ybuf):
        assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all()
    assert torch.equal(xv.cpu(), x)


@pytest.mark.gpu
def test_gate_on_gpu_tensors(device):
    assert S.afno_mlp_available(torch.zeros(1, 4, 4, 128, device=device), 8)
    assert not S.afno_mlp_available(torch.zeros(1, 4, 4, 320, device=device), 8)  # block size 40
    assert not S.afno_mlp_available(torch.zeros(1, 4, 4, 64, device=device), 8)   # block size 8


def _strict():
    prev = utils.strict_mode(True)
    S.fallback_reset()
    return prev


@pytest.mark.gpu
@pytest.mark.parametrize("fraction", [1.0, 0.5])
def test_afno2d_amd_non_instance_shape(device, fraction):
    """H = 12 has no fused instance: before afno_mlp this raised under strict_mode (torch.baddbmm fallback)."""
    torch.manual_seed(31)
    B, H, W, C, nb = 2, 12, 24, 128, 8
    x = torch.randn(B, H, W, C)
    w1, b1, w2, b2 = _params(nb, C // nb, seed=3)
    ref = afno2d_reference(x, w1, b1, w2, b2, nb, 0.01, fraction)
    xd = x.to(device)
    wd = [t.to(device) for t in (w1, b1, w2, b2)]
    assert not S.afno_fused_available(xd, nb) and S.afno_mlp_available(xd, nb)
    prev = _strict()
    try:
        out = afno2d_amd(xd, *wd, nb, 0.01, fraction)
        outb = afno2d_amd(xd.to(torch.bfloat16), *wd, nb, 0.01, fraction)
        assert S.fallback_counts() == {}
    finally:
        utils.strict_mode(prev)
    assert outb.dtype == torch.bfloat16
    e32, e16 = rel_l2(out, ref), rel_l2(outb.float(), ref)
    print(f"MEASURED afno2d_mlp fraction={fraction} fp32 {e32:.3e} bf16 {e16:.3e}")
    assert e32 < 1e-5
    assert e16 < 1e-2


def _small_net(device, fraction):
    torch.manual_seed(41)
    cfg = AFNOConfig(img_size=(96, 192), embed_dim=128, depth=2, num_blocks=4, hard_thresholding_fraction=fraction)
    m = AFNONet(cfg, backend="torch").to(device).eval()
    x = torch.randn(1, cfg.in_chans, *cfg.img_size, device=device)
    return m, x


@pytest.mark.gpu
@pytest.mark.parametrize("fraction", [1.0, 0.5])
def test_afnonet_depth2_strict(device, fraction):
    """embed 128 at 4 blocks (block size 32, hidden 512) on a 12 x 24 token grid: filter on afno_mlp, MLP on the hand
    GEMM, no fallbacks, against the torch backend."""
    m, x = _small_net(device, fraction)
    with torch.no_grad():
        ref = m(x)
        prev = _strict()
        try:
            out = m.set_backend("amd")(x)
            outb = m.to(torch.bfloat16)(x.to(torch.bfloat16))
            assert S.fallback_counts() == {}
        finally:
            utils.strict_mode(prev)
    e32, e16 = rel_l2(out, ref), rel_l2(outb.float(), ref)
    print(f"MEASURED afnonet_mlp fraction={fraction} fp32 {e32:.3e} bf16 {e16:.3e}")
    assert e32 < 5e-5
    assert e16 < 2e-2


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_afnonet_graph_capture(device, dtype):
    m, x = _small_net(device, 1.0)
    m = m.set_backend("amd").to(dtype)
    x = x.to(dtype)
    with torch.no_grad():
        eager = m(x).clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = m(x)
        outs = []
        for _ in range(2):
            g.replay()
            torch.cuda.synchronize()
            outs.append(y.clone())
    assert torch.equal(outs[0], eager) and torch.equal(outs[1], eager)


@pytest.mark.gpu
def test_determinism(device):
    x, (w1, b1, w2, b2), nb, _, _ = _case(80, 200)
    xd = x.to(device)
    for split in (False, True):
        packed = [t.to(device) for t in S.pack_afno_weights(w1, b1, w2, b2, split)]
        a = torch.ops.amd_dft.afno_mlp(xd, *packed, 0.01)
        b = torch.ops.amd_dft.afno_mlp(xd, *packed, 0.01)
        assert torch.equal(a, b)
