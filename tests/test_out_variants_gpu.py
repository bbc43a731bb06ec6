"""The table of tests/test_out_variants.py on the device: every family's ``_out`` op writes into a view inside a
larger buffer exactly what the allocating op returns (both run one launch path, and no kernel here uses atomics, so
bit for bit), leaves the buffer around the view alone, and refuses an ``out`` that starts off the boundary its
kernel's stores need, or that is not on the device."""
import math

import pytest
import torch

from test_out_variants import BF, F32, ROWS, ops, row_id, to

_BITS = {BF: (torch.int16, 0x7FC1), F32: (torch.int32, 0x7FC0_1234)}  # a NaN of each dtype, as an integer
PAD = 64  # elements around the view: the aligned view starts 128 (bf16) or 256 (fp32) bytes into an allocation


def _view(device, row, offset):
    """(bits, view): an integer buffer of one fixed NaN pattern and the row's result as a view ``offset`` elements
    past its first PAD elements."""
    idt, pattern = _BITS[row.dtype]
    n = math.prod(row.shape)
    bits = torch.full((n + 2 * PAD,), pattern, dtype=idt, device=device)
    return bits, bits.view(row.dtype)[PAD + offset:PAD + offset + n].view(row.shape)


def _outside_untouched(bits, row, offset):
    n, pattern = math.prod(row.shape), _BITS[row.dtype][1]
    b = bits.cpu()
    return bool((b[:PAD + offset] == pattern).all()) and bool((b[PAD + offset + n:] == pattern).all())


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_out_into_a_view_gpu(device, row):
    op, op_out, args = getattr(ops, row.op), getattr(ops, row.op + "_out"), to(row.args(), device)
    ref = op(*args)
    assert ref.shape == row.shape and ref.dtype == row.dtype and torch.isfinite(ref).all()
    bits, view = _view(device, row, 0)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    assert op_out(*args, view) is view
    assert torch.equal(view, ref)
    assert _outside_untouched(bits, row, 0)
    # one element further: off the boundary of every family whose stores are wider than an element
    bits, view = _view(device, row, 1)
    if row.align > view.element_size():
        assert view.data_ptr() % row.align != 0
        with pytest.raises(RuntimeError, match=rf"\b{row.op}_out: out must start on a {row.align}-byte boundary"):
            op_out(*args, view)
        torch.cuda.synchronize()
        assert bool((bits.cpu() == _BITS[row.dtype][1]).all())  # refused before any launch
    else:  # fno_pointwise (per-element I/O off the vector boundary) and disco (element stores)
        assert op_out(*args, view) is view
        assert torch.equal(view, ref)
        assert _outside_untouched(bits, row, 1)
    with pytest.raises(RuntimeError, match=rf"\b{row.op}_out: "):
        op_out(*args, torch.empty(row.shape, dtype=row.dtype))
