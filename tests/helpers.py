import math

import torch


def _as_f64(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().to("cpu")
    if t.is_complex():
        return torch.view_as_real(t.to(torch.complex128))
    return t.to(torch.float64)


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    """Relative L2 error ||a - b|| / ||b|| (complex tensors compared as (re, im) pairs)."""
    a, b = _as_f64(a), _as_f64(b)
    if a.shape != b.shape and a.shape[:-1] == b.shape and a.shape[-1] == 2:
        b = torch.stack([b, torch.zeros_like(b)], -1)
    den = b.norm().item()
    num = (a - b).norm().item()
    return num / den if den > 0 else num


def per_signal_rel_l2(a: torch.Tensor, b: torch.Tensor, dim: int, pairs: bool = False):
    """Relative L2 error of every transformed 1-D line on its own: (max over signals, flat index
    of the worst signal among the lines in row-major order of the other dims).  ``dim`` is the
    transformed axis (non-negative, of the logical shape); ``pairs`` says that real inputs carry a
    trailing (re, im) dim, which belongs to the line (complex tensors always do).  An error
    confined to one tile cannot be averaged away, as it can in the global ``rel_l2``."""
    pairs = pairs or a.is_complex() or b.is_complex()
    a, b = _as_f64(a), _as_f64(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if pairs:
        a, b = a.movedim(-1, 0), b.movedim(-1, 0)
        dim += 1
    a = a.movedim(dim, 0).reshape(a.shape[dim] * (2 if pairs else 1), -1)
    b = b.movedim(dim, 0).reshape(b.shape[dim] * (2 if pairs else 1), -1)
    num = (a - b).norm(dim=0)
    den = b.norm(dim=0)
    err = torch.where(den > 0, num / den, num)
    worst = int(err.argmax())
    return float(err[worst]), worst


def _smooth_at_least(n: int) -> int:
    m = n
    while True:
        k = m
        for p in (2, 3, 5):
            while k % p == 0:
                k //= p
        if k == 1:
            return m
        m += 1


def long_fft_tol(n: int, limit: int = 6552) -> float:
    """Error model of the long-length compositions (csrc/ops/dft_ops.cpp:151-238), rel-L2 vs fp64,
    eps = 2^-24 (fp32 unit roundoff):
      * four-step / LDS-resident: eps (log2 n + 2 + sqrt(p)), p = largest prime factor of n
        (radix-r Stockham passes add ~eps per level, the fp32 twiddle multiply ~2 eps, and a
        prime factor above the specialised radices runs as a direct p-point DFT: ~eps sqrt(p));
      * Bluestein (n prime above the LDS limit): eps (3 log2 M + 3), M = the smallest 2,3,5-smooth
        length >= 2n - 1 (three chained M-point FFTs plus three complex products).
    The tolerance is 2x the model; measured errors sit 6-18x below it on MI355X
    (scripts/diag/long_fft_errors.py: 1.3e-7 .. 5.1e-7, 1.5e-6 for n = 8198 = 2 * 4099)."""
    eps = 2.0 ** -24
    p, k, f = 1, n, 2
    while f * f <= k:
        while k % f == 0:
            p, k = max(p, f), k // f
        f += 1
    p = max(p, k) if k > 1 else p
    if n <= limit or p < n:  # LDS-resident or four-step
        return 2 * eps * (math.log2(n) + 2 + math.sqrt(p))
    m = _smooth_at_least(2 * n - 1)
    return 2 * eps * (3 * math.log2(m) + 3)
