"""Spherical harmonic transforms (SHT) for spherical FNO / FourCastNet-v2 style models.

A real SHT is a truncated real FFT along longitude followed by a Legendre transform along latitude.  The first
half is the pruned ``r2c`` / ``c2r`` of :mod:`.dft`; the second is the ``legendre`` op
(``csrc/spectral/legendre.hip``: a per-mode real matrix applied along latitude to the complex spectrum on MFMA:
bf16x3 with fp32 in and out, or plain bf16 operands with bf16 in and out).

Conventions (the torch-harmonics "ortho" ones, so weights trained there carry over):

* grid: ``nlat`` colatitudes theta_k, north to south, and ``nlon`` longitudes phi_j = 2 pi j / nlon.
  ``"legendre-gauss"``: cos theta_k are the Gauss-Legendre nodes; ``"equiangular"``: theta_k = pi k / (nlat - 1),
  poles included, Clenshaw-Curtis weights.  Both sets of weights sum to 2.
* basis: the associated Legendre functions Pb_l^m with the Condon-Shortley phase, normalised so that
  2 pi int Pb_l^m Pb_l'^m dx = delta_ll' (Pb_0^0 = 1 / sqrt(4 pi)).
* forward: F[k, m] = (2 pi / nlon) sum_j f[k, j] exp(-i m phi_j) for 0 <= m < mmax, then
  c[l, m] = sum_k w_k Pb_l^m(cos theta_k) F[k, m] for 0 <= l < lmax (zero where l < m) -> ``[..., lmax, mmax, 2]``.
* inverse: F[k, m] = sum_l Pb_l^m(cos theta_k) c[l, m], then the Hermitian-completed sum over m: an unnormalised
  C2R from ``mmax`` stored modes (``torch.fft.irfft(..., n=nlon, norm="forward")``).
* defaults: ``lmax = nlat``, ``mmax = min(lmax, nlon // 2 + 1)``.

Vector transforms (``vsht`` / ``ivsht``, the pair torch-harmonics calls ``RealVectorSHT`` / ``InverseRealVectorSHT``,
same layout and names): a tangential field v = (v_theta, v_phi) [..., 2, nlat, nlon], component 0 colatitudinal, is
expanded in the vector harmonics Psi = grad Y (spheroidal) and Phi = r x grad Y (toroidal, r the unit radial vector:
this fixes the sign of the toroidal part) -> [..., 2, lmax, mmax, 2].  With the derivative tables
D0[m, l, k] = d Pb_l^m / d theta and D1[m, l, k] = m Pb_l^m / sin theta (``vector_legendre_tables``; both zero for
l < max(m, 1)), U, V the scaled longitude transforms of the two components and W_j = w_k D_j / (l (l + 1)):

* forward: s[l, m] = sum_k W0 U - i W1 V,  t[l, m] = sum_k W0 V + i W1 U;
* inverse: U[k, m] = sum_l D0 s - i D1 t,  V[k, m] = sum_l D0 t + i D1 s, then the C2R of ``isht`` per component.

Both are the ``legendre_vec`` op (``csrc/spectral/legendre.hip``, ``VEC``): one kernel pass over both tables and both
components.  ``vsht`` of the gradient (d f / d theta, (1 / sin theta) d f / d phi) of a band-limited scalar f is
s = sht(f) for l >= 1, t = 0.  ``ivsht(vsht(v))`` reproduces a band-limited v where the quadrature is exact for the
products involved: ``legendre-gauss`` up to lmax = nlat, ``equiangular`` up to lmax = (nlat + 1) / 2.

Precision follows the input: fp32 (the tables are built in fp64 on the host and rounded once to fp32; the Legendre
kernel runs the bf16x3 split, ~1e-6) or bf16 (the tables are ``bf16(fp32 table)``, the spectrum between the longitude
FFT and ``legendre`` is bf16, the kernel multiplies the bf16 operands as they are with fp32 accumulation and rounds
once at the store; a transform is good to about 3e-3 per field, bound 2e-2).  Complex bf16 does not exist, so bf16
coefficients are always real tensors with a trailing re/im dim.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .._loader import load_plugins
from .dft import _from_complex

__all__ = ["legendre_tables", "sht", "isht", "sht_tables", "legendre_split", "GRIDS", "quadrature", "colatitudes",
           "vector_legendre_tables", "vsht", "ivsht", "vsht_tables"]

GRIDS = ("equiangular", "legendre-gauss")


def _ops():
    load_plugins()
    return torch.ops.amd_dft


def _clenshaw_curtis(n: int) -> Tuple[np.ndarray, np.ndarray]:
    """cos theta_k at theta_k = pi k / (n - 1) and the Clenshaw-Curtis weights, closed form:
    w_k = c_k / N (1 - sum_{j=1}^{N/2} b_j / (4 j^2 - 1) cos(2 j theta_k)), N = n - 1, c = 1 at the poles else 2,
    b_j = 1 at j = N / 2 else 2."""
    if n < 2:
        raise ValueError("the equiangular grid needs nlat >= 2")
    N = n - 1
    theta = np.pi * np.arange(n, dtype=np.float64) / N
    w = np.ones(n, dtype=np.float64)
    for j in range(1, N // 2 + 1):
        b = 1.0 if 2 * j == N else 2.0
        w -= b / (4.0 * j * j - 1.0) * np.cos(2.0 * j * theta)
    c = np.full(n, 2.0)
    c[0] = c[-1] = 1.0
    return np.cos(theta), c * w / N


def quadrature(nlat: int, grid: str = "equiangular") -> Tuple[np.ndarray, np.ndarray]:
    """(nodes cos theta_k [nlat], north to south; weights w_k [nlat], summing to 2) of a latitude grid, float64."""
    if grid == "legendre-gauss":
        x, w = np.polynomial.legendre.leggauss(nlat)
        return x[::-1].copy(), w[::-1].copy()
    if grid == "equiangular":
        return _clenshaw_curtis(nlat)
    raise ValueError(f"grid must be one of {GRIDS}, got {grid!r}")


def colatitudes(nlat: int, grid: str = "equiangular") -> Tuple[np.ndarray, np.ndarray]:
    """(colatitudes theta_k [nlat], north to south; weights w_k [nlat]) of ``quadrature``'s grid.  The equiangular
    theta_k = pi k / (nlat - 1) are taken as they are defined, not through arccos, which loses digits at the poles."""
    x, w = quadrature(nlat, grid)
    if grid == "equiangular":
        return np.pi * np.arange(nlat, dtype=np.float64) / (nlat - 1), w
    return np.arccos(x), w


def legendre_tables(nlat: int, lmax: int, mmax: int, grid: str = "equiangular"):
    """(nodes cos theta_k [nlat], north to south; weights w_k [nlat]; Pb [mmax, lmax, nlat]), all float64 numpy.

    Pb[m, l, k] = Pb_l^m(cos theta_k), zero where l < m, by the standard recurrences carried in fp64:
    Pb_m^m = -sqrt((2m + 1) / (2m)) sin(theta) Pb_{m-1}^{m-1}, then in l
    Pb_l^m = sqrt((4 l^2 - 1) / (l^2 - m^2)) (x Pb_{l-1}^m - sqrt(((l - 1)^2 - m^2) / (4 (l - 1)^2 - 1)) Pb_{l-2}^m)."""
    x, w = quadrature(nlat, grid)
    if lmax < 1 or mmax < 1:
        raise ValueError("lmax and mmax must be >= 1")
    s = np.sqrt(np.maximum(0.0, 1.0 - x * x))
    P = np.zeros((mmax, lmax, nlat), dtype=np.float64)
    pmm = np.full(nlat, 1.0 / math.sqrt(4.0 * math.pi))
    for m in range(min(mmax, lmax)):
        if m > 0:
            pmm = -math.sqrt((2.0 * m + 1.0) / (2.0 * m)) * s * pmm
        P[m, m] = pmm
        for l in range(m + 1, lmax):
            a = math.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
            b = math.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0)) if l > m + 1 else 0.0
            P[m, l] = a * (x * P[m, l - 1] - (b * P[m, l - 2] if l > m + 1 else 0.0))
    return x, w, P


def legendre_split(table: torch.Tensor) -> torch.Tensor:
    """A Legendre table [M, R, Q] as the kernel reads it: zero-padded to [M, ceil16(R), ceil32(Q)] and split into
    bf16 (hi, lo) planes -> [2, M, Rp, Qp] (``split_bf16(rows=False)``).  A bf16 table is its own single plane:
    zero-padded -> [1, M, Rp, Qp]."""
    M, R, Q = table.shape
    if table.dtype == torch.bfloat16:
        return F.pad(table, (0, -Q % 32, 0, -R % 16)).contiguous().unsqueeze(0)
    tp = F.pad(table.float(), (0, -Q % 32, 0, -R % 16)).contiguous()
    return _ops().split_bf16(tp, False)


class _Tables:
    """The operands of one (grid, truncation) on one device in one precision: ``fwd`` [mmax, lmax, nlat] = w_k Pb,
    ``inv`` [mmax, nlat, lmax] = Pb transposed, and on a GPU their split forms.  ``like``: the fp32 tables to round
    to bf16 (the bf16 operands are ``bf16(fp32 table)``)."""

    def __init__(self, nlat, nlon, lmax, mmax, grid, device, like: "Optional[_Tables]" = None):
        if like is not None:
            self.fwd, self.inv = like.fwd.to(torch.bfloat16), like.inv.to(torch.bfloat16)
        else:
            _, w, P = legendre_tables(nlat, lmax, mmax, grid)
            self.fwd = torch.from_numpy(P * w[None, None, :]).float().contiguous().to(device)
            self.inv = torch.from_numpy(np.ascontiguousarray(P.transpose(0, 2, 1))).float().to(device)
        cuda = torch.device(device).type == "cuda"
        self.fwd_split = legendre_split(self.fwd) if cuda else None
        self.inv_split = legendre_split(self.inv) if cuda else None


_CACHE: dict = {}


def sht_tables(nlat: int, nlon: int, lmax: int, mmax: int, grid: str, device,
               dtype: torch.dtype = torch.float32) -> _Tables:
    """Tables cached per (nlat, nlon, lmax, mmax, grid, device) and dtype (fp32 or bf16; the bf16 entry is the fp32
    one rounded); they live as long as the process, so a captured hipGraph that reads them stays valid."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"sht_tables: dtype must be float32 or bfloat16, got {dtype}")
    key = (int(nlat), int(nlon), int(lmax), int(mmax), grid, str(torch.device(device)))
    t = _CACHE.get(key)
    if t is None:
        t = _CACHE[key] = _Tables(nlat, nlon, lmax, mmax, grid, device)
    if dtype == torch.bfloat16:
        key, t32 = key + (dtype,), t
        t = _CACHE.get(key)
        if t is None:
            t = _CACHE[key] = _Tables(nlat, nlon, lmax, mmax, grid, device, like=t32)
    return t


def _defaults(nlat: int, nlon: int, lmax: Optional[int], mmax: Optional[int]) -> Tuple[int, int]:
    lmax = int(lmax) if lmax is not None else nlat
    mmax = int(mmax) if mmax is not None else min(lmax, nlon // 2 + 1)
    if not 1 <= mmax <= nlon // 2 + 1:
        raise ValueError(f"mmax must be in [1, nlon // 2 + 1 = {nlon // 2 + 1}], got {mmax}")
    if lmax < 1:
        raise ValueError("lmax must be >= 1")
    return lmax, mmax


def sht(x: torch.Tensor, lmax: Optional[int] = None, mmax: Optional[int] = None,
        grid: str = "equiangular") -> torch.Tensor:
    """Forward real SHT of ``x`` [..., nlat, nlon] (fp32 or bf16) -> coefficients [..., lmax, mmax, 2] (trailing
    re/im) of the same dtype.

    R2C along longitude keeping ``mmax`` modes, scaled by 2 pi / nlon, then the forward Legendre transform
    (``legendre`` with ``tri=1``: rows l < m are zero).  The same two ops run on CPU tensors (ATen kernels)."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"sht: x must be float32 or bfloat16, got {x.dtype}")
    nlat, nlon = int(x.shape[-2]), int(x.shape[-1])
    lmax, mmax = _defaults(nlat, nlon, lmax, mmax)
    t = sht_tables(nlat, nlon, lmax, mmax, grid, x.device, x.dtype)
    ops = _ops()
    xf = ops.r2c(x, [x.dim() - 1], 2.0 * math.pi / nlon, [mmax, 0], x.dtype)  # [..., nlat, mmax, 2]
    return ops.legendre(xf, t.fwd, t.fwd_split, 1)


def isht(c: torch.Tensor, nlat: int, nlon: int, grid: str = "equiangular") -> torch.Tensor:
    """Inverse real SHT of ``c`` [..., lmax, mmax, 2] (fp32 or bf16; or complex64 [..., lmax, mmax]) ->
    [..., nlat, nlon] of the same real dtype.

    The inverse Legendre transform (``legendre`` with ``tri=2``: columns l < m are zero), then an unnormalised C2R
    along longitude from the ``mmax`` stored modes."""
    c = _from_complex(c)
    if c.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"isht: c must be float32 / complex64 or bfloat16 (trailing re/im), got {c.dtype}")
    lmax, mmax = int(c.shape[-3]), int(c.shape[-2])
    _defaults(nlat, nlon, lmax, mmax)
    t = sht_tables(nlat, nlon, lmax, mmax, grid, c.device, c.dtype)
    ops = _ops()
    xf = ops.legendre(c, t.inv, t.inv_split, 2)  # [..., nlat, mmax, 2]
    return ops.c2r(xf, [xf.dim() - 2], [nlon], 1.0, [mmax, 0], c.dtype)


# ------------------------------------------------------------------------------------------------ vector transforms
def vector_legendre_tables(nlat: int, lmax: int, mmax: int, grid: str = "equiangular"):
    """(nodes [nlat], weights [nlat], D0 [mmax, lmax, nlat], D1 [mmax, lmax, nlat]), all float64 numpy.

    D0[m, l, k] = d Pb_l^m / d theta = -1/2 (sqrt((l + m)(l - m + 1)) Pb_l^{m-1} - sqrt((l - m)(l + m + 1)) Pb_l^{m+1})
    D1[m, l, k] = m Pb_l^m / sin theta
                = -1/2 sqrt((2l + 1) / (2l - 1)) (sqrt((l - m)(l - m - 1)) Pb_{l-1}^{m+1} + sqrt((l + m)(l + m - 1)) Pb_{l-1}^{m-1})
    with Pb_l^{-1} = -Pb_l^1, from the recurrence of ``legendre_tables`` carried one order further.  Rows l < max(m, 1)
    are zero and so is the m = 0 plane of D1; D1 never divides by sin theta, so it is finite at the poles."""
    x, w, P = legendre_tables(nlat, lmax, mmax + 1, grid)  # orders 0 .. mmax

    def order(m):  # Pb^m as [lmax, nlat], m >= -1
        return P[m] if m >= 0 else -P[1]

    l = np.arange(lmax, dtype=np.float64)[:, None]
    D0 = np.zeros((mmax, lmax, nlat), dtype=np.float64)
    D1 = np.zeros((mmax, lmax, nlat), dtype=np.float64)
    for m in range(min(mmax, lmax)):
        lo, hi = order(m - 1), order(m + 1)
        cm = np.sqrt(np.maximum(0.0, (l + m) * (l - m + 1.0)))
        cp = np.sqrt(np.maximum(0.0, (l - m) * (l + m + 1.0)))
        D0[m] = -0.5 * (cm * lo - cp * hi)
        if m >= 1:
            am = np.sqrt(np.maximum(0.0, (l - m) * (l - m - 1.0)))
            ap = np.sqrt(np.maximum(0.0, (l + m) * (l + m - 1.0)))
            D1[m, 1:] = (-0.5 * np.sqrt((2.0 * l + 1.0) / np.maximum(1.0, 2.0 * l - 1.0)))[1:] * (
                am[1:] * hi[:-1] + ap[1:] * lo[:-1])
        D0[m, :max(m, 1)] = 0.0
        D1[m, :max(m, 1)] = 0.0
    return x, w, D0, D1


class _VecTables:
    """The operands of ``vsht`` / ``ivsht`` for one (grid, truncation) on one device in one precision:
    ``fwd_a``, ``fwd_b`` [mmax, lmax, nlat] = w_k D_j / (l (l + 1)), ``inv_a``, ``inv_b`` [mmax, nlat, lmax] = D_j
    transposed, and on a GPU their split forms.  ``like``: the fp32 tables to round to bf16."""

    NAMES = ("fwd_a", "fwd_b", "inv_a", "inv_b")

    def __init__(self, nlat, nlon, lmax, mmax, grid, device, like: "Optional[_VecTables]" = None):
        if like is not None:
            for n in self.NAMES:
                setattr(self, n, getattr(like, n).to(torch.bfloat16))
        else:
            _, w, D0, D1 = vector_legendre_tables(nlat, lmax, mmax, grid)
            l = np.arange(lmax, dtype=np.float64)
            norm = np.where(l > 0, 1.0 / np.maximum(1.0, l * (l + 1.0)), 0.0)[None, :, None] * w[None, None, :]
            for n, D in (("fwd_a", D0 * norm), ("fwd_b", D1 * norm),
                         ("inv_a", D0.transpose(0, 2, 1)), ("inv_b", D1.transpose(0, 2, 1))):
                setattr(self, n, torch.from_numpy(np.ascontiguousarray(D)).float().to(device))
        cuda = torch.device(device).type == "cuda"
        for n in self.NAMES:
            setattr(self, n + "_split", legendre_split(getattr(self, n)) if cuda else None)


def vsht_tables(nlat: int, nlon: int, lmax: int, mmax: int, grid: str, device,
                dtype: torch.dtype = torch.float32) -> _VecTables:
    """The vector tables, cached like ``sht_tables`` (the same key plus a vector tag)."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"vsht_tables: dtype must be float32 or bfloat16, got {dtype}")
    key = (int(nlat), int(nlon), int(lmax), int(mmax), grid, str(torch.device(device)), "vector")
    t = _CACHE.get(key)
    if t is None:
        t = _CACHE[key] = _VecTables(nlat, nlon, lmax, mmax, grid, device)
    if dtype == torch.bfloat16:
        key, t32 = key + (dtype,), t
        t = _CACHE.get(key)
        if t is None:
            t = _CACHE[key] = _VecTables(nlat, nlon, lmax, mmax, grid, device, like=t32)
    return t


def vsht(x: torch.Tensor, lmax: Optional[int] = None, mmax: Optional[int] = None,
         grid: str = "equiangular") -> torch.Tensor:
    """Forward vector SHT of ``x`` [..., 2, nlat, nlon] (fp32 or bf16; component 0 = v_theta, 1 = v_phi) ->
    [..., 2, lmax, mmax, 2] of the same dtype (component 0 spheroidal, 1 toroidal; trailing re/im).

    One R2C along longitude over both components (as ``sht``), then ``legendre_vec`` with ``tri=1``."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"vsht: x must be float32 or bfloat16, got {x.dtype}")
    if x.dim() < 3 or x.shape[-3] != 2:
        raise ValueError(f"vsht: x must be [..., 2, nlat, nlon], got {tuple(x.shape)}")
    nlat, nlon = int(x.shape[-2]), int(x.shape[-1])
    lmax, mmax = _defaults(nlat, nlon, lmax, mmax)
    t = vsht_tables(nlat, nlon, lmax, mmax, grid, x.device, x.dtype)
    ops = _ops()
    xf = ops.r2c(x, [x.dim() - 1], 2.0 * math.pi / nlon, [mmax, 0], x.dtype)  # [..., 2, nlat, mmax, 2]
    return ops.legendre_vec(xf, t.fwd_a, t.fwd_b, t.fwd_a_split, t.fwd_b_split, 1)


def ivsht(c: torch.Tensor, nlat: int, nlon: int, grid: str = "equiangular") -> torch.Tensor:
    """Inverse vector SHT of ``c`` [..., 2, lmax, mmax, 2] (fp32 or bf16; or complex64 [..., 2, lmax, mmax]) ->
    [..., 2, nlat, nlon] of the same real dtype.

    ``legendre_vec`` with ``tri=2``, then one unnormalised C2R along longitude over both components (as ``isht``)."""
    c = _from_complex(c)
    if c.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"ivsht: c must be float32 / complex64 or bfloat16 (trailing re/im), got {c.dtype}")
    if c.dim() < 4 or c.shape[-4] != 2 or c.shape[-1] != 2:
        raise ValueError(f"ivsht: c must be [..., 2, lmax, mmax, 2], got {tuple(c.shape)}")
    lmax, mmax = int(c.shape[-3]), int(c.shape[-2])
    _defaults(nlat, nlon, lmax, mmax)
    t = vsht_tables(nlat, nlon, lmax, mmax, grid, c.device, c.dtype)
    ops = _ops()
    xf = ops.legendre_vec(c, t.inv_a, t.inv_b, t.inv_a_split, t.inv_b_split, 2)  # [..., 2, nlat, mmax, 2]
    return ops.c2r(xf, [xf.dim() - 2], [nlon], 1.0, [mmax, 0], c.dtype)
