"""The nine op families with an ``_out`` op, one table row per family and dtype: what every ``_out`` op promises
whatever the family, on CPU and meta tensors.  The device tier of the same table: tests/test_out_variants_gpu.py.

1. ``op_out(..., out)`` returns ``out`` itself, holding ``op(...)`` bit for bit.
2. An ``out`` that is not what ``op`` returns -- wrong shape, wrong dtype, a non-contiguous view, a tensor on the meta
   device -- raises under the ``_out`` op's name; it is never copied into.
3. On meta tensors ``op`` returns the result's shape and dtype and ``op_out`` returns ``out``.

Shapes are the smallest of each family's own tests; what the results are is checked there."""
from collections import namedtuple

import pytest
import torch

import tensorrt_dft_plugins_amd as tdp
from tensorrt_dft_plugins_amd.ops import disco as D
from tensorrt_dft_plugins_amd.ops import spectral as SP

tdp.load_plugins()
ops = torch.ops.amd_dft
F32, BF = torch.float32, torch.bfloat16

# op: the family's name; args: () -> the op's arguments on the CPU (built once); shape, dtype: what the op returns;
# align: bytes the device op needs of out's start (0: any element)
Row = namedtuple("Row", "op args shape dtype align")
_ARGS = {}


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _afno_mlp(dt):  # block size 16, 9 tokens
    nb, bs = 8, 16
    w1, w2 = 0.05 * _randn(1, 2, nb, bs, bs), 0.05 * _randn(2, 2, nb, bs, bs)
    b1, b2 = 0.05 * _randn(3, 2, nb, bs), 0.05 * _randn(4, 2, nb, bs)
    return (_randn(5, 9, nb * bs, 2), *SP.pack_afno_weights(w1, b1, w2, b2), 0.01)


def _fno_mix(dt):
    return _randn(6, 3, 5, 11, 2).to(dt), _randn(7, 5, 7, 11, 2).to(dt), 0


def _fno_pointwise(dt):
    return _randn(8, 2, 9, 5, 7).to(dt), _randn(9, 2, 5, 5, 7).to(dt), _randn(10, 9, 5), _randn(11, 9), True


def _fno_c2r_pw(dt):  # the wide kernel's smallest case in tests/test_fno_tail_wide.py: 5 modes
    yw, x, wc = _randn(12, 1, 40, 2, 5, 2) / 10 ** 0.5, _randn(13, 1, 7, 2, 72), _randn(14, 40, 7) / 7 ** 0.5
    return yw, x.to(dt), wc, None, False


def _legendre(dt):
    return _randn(15, 2, 45, 13, 2).to(dt), (_randn(16, 13, 23, 45) / 45 ** 0.5).to(dt), None, 0


def _legendre_vec(dt):  # tests/test_vsht.py OP_CASES[0]
    x, ta, tb = _randn(17, 3, 2, 33, 9, 2), _randn(18, 9, 20, 33) / 33 ** 0.5, _randn(19, 9, 20, 33) / 33 ** 0.5
    return x.to(dt), ta.to(dt), tb.to(dt), None, None, 0


def _disco(dt):  # tests/test_disco.py GRID_CASES[0]: 13 x 24 equiangular onto itself, three radial basis functions
    rp, idx, val = (torch.from_numpy(a) for a in D.disco_tables((13, 24), (13, 24), 3, "equiangular", "equiangular"))
    return _randn(20, 2, 13, 24).to(dt), rp, idx, val, 3, 13, 24


def _sfno_mix(dt):
    return _randn(21, 3, 5, 12, 9, 2).to(dt), (_randn(22, 5, 7, 12, 2) / 5 ** 0.5).to(dt), None, 0


def _instance_norm(dt):
    return _randn(23, 2, 3, 7, 9).to(dt), _randn(24, 3), _randn(25, 3), 1e-5


# alignment: the table of the ops' contract (csrc/ops/spectral_ops.cpp): one (re, im) pair for the complex results,
# one element for disco, 16 bytes for the vector stores of afno_mlp, fno_c2r_pw and instance_norm
_FAMILIES = [
    ("afno_mlp", _afno_mlp, (9, 128, 2), {F32: 16}),
    ("fno_mix", _fno_mix, (3, 7, 11, 2), {F32: 8, BF: 4}),
    ("fno_pointwise", _fno_pointwise, (2, 9, 5, 7), {F32: 0, BF: 0}),
    ("fno_c2r_pw", _fno_c2r_pw, (1, 40, 2, 72), {F32: 16, BF: 16}),
    ("legendre", _legendre, (2, 23, 13, 2), {F32: 8, BF: 4}),
    ("legendre_vec", _legendre_vec, (3, 2, 20, 9, 2), {F32: 8, BF: 4}),
    ("disco", _disco, (2, 3, 13, 24), {F32: 4, BF: 2}),
    ("sfno_mix", _sfno_mix, (3, 7, 12, 9, 2), {F32: 8, BF: 4}),
    ("instance_norm", _instance_norm, (2, 3, 7, 9), {F32: 16, BF: 16}),
]


def _cached(op, make, dt):
    def args():
        if (op, dt) not in _ARGS:
            _ARGS[op, dt] = make(dt)
        return _ARGS[op, dt]
    return args


ROWS = [Row(op, _cached(op, make, dt), shape, dt, align)
        for op, make, shape, aligns in _FAMILIES for dt, align in aligns.items()]
row_id = lambda r: f"{r.op}-{'bf16' if r.dtype == BF else 'fp32'}"  # noqa: E731


def to(args, device):
    return tuple(a.to(device) if isinstance(a, torch.Tensor) else a for a in args)


def test_the_table_holds_every_family():
    assert {r.op for r in ROWS} == {"afno_mlp", "fno_mix", "fno_pointwise", "fno_c2r_pw", "legendre", "legendre_vec",
                                    "disco", "sfno_mix", "instance_norm"}
    assert len(ROWS) == 17  # fp32 and bf16 of each but afno_mlp, which is fp32 only


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_out_is_the_allocating_ops_result(row):
    op, op_out, args = getattr(ops, row.op), getattr(ops, row.op + "_out"), row.args()
    ref = op(*args)
    assert ref.shape == row.shape and ref.dtype == row.dtype
    assert torch.isfinite(ref).all() and ref.float().abs().max() > 0
    out = torch.full(row.shape, float("nan"), dtype=row.dtype)
    assert op_out(*args, out) is out
    assert torch.equal(out, ref)


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_out_that_is_not_the_result_raises(row):
    op_out, args = getattr(ops, row.op + "_out"), row.args()
    *lead, last = row.shape
    bad = {"shape": torch.empty(*lead, last + 1, dtype=row.dtype),
           "dtype": torch.empty(row.shape, dtype=torch.float64),
           "non-contiguous": torch.empty(*lead, 2 * last, dtype=row.dtype)[..., ::2],
           "meta": torch.empty(row.shape, dtype=row.dtype, device="meta")}
    assert bad["non-contiguous"].shape == row.shape and not bad["non-contiguous"].is_contiguous()
    for what, out in bad.items():
        with pytest.raises(RuntimeError, match=rf"\b{row.op}_out: "):
            op_out(*args, out)
            pytest.fail(f"{row.op}_out took an out of the wrong {what}")


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_meta(row):
    op, op_out, args = getattr(ops, row.op), getattr(ops, row.op + "_out"), to(row.args(), "meta")
    y = op(*args)
    assert y.device.type == "meta" and y.shape == row.shape and y.dtype == row.dtype
    out = torch.empty(row.shape, dtype=row.dtype, device="meta")
    assert op_out(*args, out) is out
