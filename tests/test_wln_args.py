"""Argument checks and result shapes of the LayerNorm-fused W-transform family, one table for the four ops.

``r2c_ln``, ``c2r_ln_add``, ``c2r_ln_add_split`` and ``c2r_ln_add_part`` build their arguments with one function, so
every op rejects the same malformed call with the same words, on the CPU and on the device, before any work.  The
table's base case is x ``[2, 8, 64]`` with X ``[2, 5, 64, 2]`` and n = 8: the smallest with ``C % 64 == 0`` and a
leading dim to mismatch.  Each row changes one argument and names a substring of the message it must raise.
The meta forms return the shapes and dtypes the CPU forms compute.
"""
import pytest
import torch

ops = torch.ops.amd_dft

F32, BF16 = torch.float32, torch.bfloat16
B, N, KM, C = 2, 8, 5, 64
OPS = ("r2c_ln", "c2r_ln_add", "c2r_ln_add_split", "c2r_ln_add_part")
C2R = OPS[1:]


def base(op, dtype=None, c=C):
    """A valid call's arguments by name; the part op takes bf16, the others fp32"""
    dtype = dtype or (BF16 if op == "c2r_ln_add_part" else F32)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, N, c, generator=g).to(dtype)
    var, mean = torch.var_mean(x.double(), dim=-1, correction=0)
    return dict(x=x, X=torch.randn(B, KM, c, 2, generator=g).to(dtype), dim=-2, n=N, keep=KM,
                stats=torch.stack([mean, torch.rsqrt(var + 1e-6)], -1).reshape(-1, 2).float(),
                g=1 + 0.1 * torch.randn(c, generator=g), b=0.1 * torch.randn(c, generator=g), out_mode=1)


def call(op, a, device="cpu"):
    d = lambda t: t.to(device)  # noqa: E731
    ln = (d(a["stats"]), d(a["g"]), d(a["b"]), None)
    if op == "r2c_ln":
        return (ops.r2c_ln(d(a["x"]), a["dim"], 1.0, a["keep"], *ln, a["x"].dtype),)
    head = (d(a["X"]), a["dim"], a["n"], 0.5, d(a["x"]), *ln)
    if op == "c2r_ln_add":
        return (ops.c2r_ln_add(*head),)
    if op == "c2r_ln_add_split":
        return tuple(ops.c2r_ln_add_split(*head, a["out_mode"]))
    return tuple(ops.c2r_ln_add_part(*head))


def _set(**kw):
    return lambda a: a.update(kw)


def _spectrum(shape):
    return lambda a: a.update(X=torch.zeros(*shape, 2, dtype=a["X"].dtype))


# (id, ops, what to change in the base case, substring of the message, base dtype or None, base channel count)
# The four rows on X against x (lead, channels, km, length) meet one check with one message, so their substrings name
# that message, not the clause that failed: each row shows that its clause is in the check.
REJECTIONS = [
    ("axis", OPS, _set(dim=0), "dim -2", None, C),
    ("gamma", OPS, lambda a: a.update(g=torch.ones(C + 1)), "per channel", None, C),
    ("stats", OPS, lambda a: a.update(stats=a["stats"][:-1]), "per token", None, C),
    ("lead", C2R, _spectrum((B + 1, KM, C)), "leading dims", None, C),
    ("channels", C2R, _spectrum((B, KM, 2 * C)), "leading dims", None, C),
    ("km", C2R, _spectrum((B, N // 2 + 2, C)), "km <= n/2+1", None, C),
    ("keep", ("r2c_ln",), _set(keep=N // 2 + 2), "exceed", None, C),
    ("length", C2R, _set(n=N + 2), "leading dims", None, C),
    ("split_bf16", ("c2r_ln_add_split",), _set(), "fp32 residual stream", BF16, C),
    ("part_fp32", ("c2r_ln_add_part",), _set(), "bf16 spectrum", F32, C),
    ("c32", ("c2r_ln_add_split", "c2r_ln_add_part"), _set(), "multiple of 64", None, 32),
    ("out_mode", ("c2r_ln_add_split",), _set(out_mode=3), "out_mode", None, C),
]
ROWS = [pytest.param(op, change, msg, dtype, c, id=f"{op}-{rid}")
        for rid, row_ops, change, msg, dtype, c in REJECTIONS for op in row_ops]


def _rejects(op, change, msg, dtype, c, device):
    a = base(op, dtype, c)
    change(a)
    with pytest.raises(RuntimeError, match=msg.replace("+", r"\+")):
        call(op, a, device)


@pytest.mark.parametrize("op,change,msg,dtype,c", ROWS)
def test_rejects_cpu(op, change, msg, dtype, c):
    _rejects(op, change, msg, dtype, c, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("op,change,msg,dtype,c", ROWS)
def test_rejects_gpu(device, op, change, msg, dtype, c):
    """The same rows on device tensors: every one raises in the host checks, before any launch"""
    _rejects(op, change, msg, dtype, c, device)


@pytest.mark.parametrize("op,out_mode", [(op, 1) for op in OPS] + [("c2r_ln_add_split", 0), ("c2r_ln_add_split", 2)])
def test_meta_results_match_cpu(op, out_mode):
    a = base(op)
    a["out_mode"] = out_mode
    got, want = call(op, a, "meta"), call(op, a)
    assert [(tuple(t.shape), t.dtype) for t in got] == [(tuple(t.shape), t.dtype) for t in want]
