"""Discrete-continuous (DISCO) convolutions on the sphere: the filter tensor and the ``disco`` op.

A DISCO convolution (Ocampo, Price, McEwen 2022; the local layer of spherical U-Nets and local spherical neural
operators) evaluates a continuous, compactly supported filter around every output point by quadrature over the
input grid.  On latitude/longitude grids the filter tensor does not depend on the output longitude, so it is a
sparse tensor Psi[p, k', k, d] applied at every output longitude with a shift.

Definition (the layout of torch-harmonics' ``DiscreteContinuousConvS2``, NOT its normalisation: published weights
do not carry over):

* grids: input ``(nlat_in, nlon_in, grid_in)``, output ``(nlat_out, nlon_out, grid_out)``, the grids of
  :mod:`.sht` (``colatitudes``: theta_k north to south, weights w_k summing to 2); ``nlon_in % nlon_out == 0``,
  ``s = nlon_in / nlon_out``; longitudes phi_j = 2 pi j / nlon_in; quadrature weight q_k = w_k 2 pi / nlon_in.
* local coordinates of an input point (theta, phi) about an output point (theta', 0) rotated to the pole:
  z = cos theta cos theta' + sin theta sin theta' cos phi, r = arccos(clamp(z, -1, 1)),
  X = cos theta' sin theta cos phi - sin theta' cos theta, Y = sin theta sin phi, gamma = atan2(Y, X) mod 2 pi.
* basis, piecewise linear: dr = theta_cutoff / nr, hat_i(r) = max(0, 1 - |r - i dr| / dr).  ``kernel_shape = nr``:
  isotropic, K = nr, psi_i = hat_i(r).  ``kernel_shape = (nr, nphi)``: anisotropic, K = 1 + (nr - 1) nphi,
  psi_0 = hat_0(r), psi_{1 + (i - 1) nphi + a} = hat_i(r) max(0, 1 - d(gamma, 2 pi a / nphi) / (2 pi / nphi)) for
  i >= 1, d the circular distance.  sum_p psi_p = 1 for r <= (nr - 1) dr, every psi is 0 for r >= theta_cutoff.
  Default ``theta_cutoff = (nr + 1) pi / (nlat_out - 1)``.
* filter tensor: Psi[p, k', k, d] = psi_p(r, gamma) q_k at phi = 2 pi d / nlon_in, only where psi_p > 0; with
  ``normalize`` divided by A_k' = sum_{p, k, d} Psi[p, k', k, d], so a constant field gives sum_p y_p = 1.
* convolution: y[b, c, p, k', j'] = sum_{k, d} Psi[p, k', k, d] x[b, c, k, (d + s j') mod nlon_in] (the ``disco``
  op, ``csrc/spectral/disco.hip``), then out[b, o, k', j'] = sum_{c, p} W[o, c, p] y[b, c, p, k', j'] + bias[o].

Transposed (upsampling) convolution (the layout of torch-harmonics' ``DiscreteContinuousConvTransposeS2``, NOT its
normalisation), same grids of :mod:`.sht`, local coordinates, basis and K:

* grids: input (coarse) ``(nlat_in, nlon_in, grid_in)``, output (fine) ``(nlat_out, nlon_out, grid_out)``;
  ``nlon_out % nlon_in == 0``, ``s = nlon_out / nlon_in`` (1 allowed); input quadrature weight
  q'_k' = w'_k' 2 pi / nlon_in.
* filter: centred on the input point (theta'_k', 2 pi j' / nlon_in), evaluated at the output point
  (theta_k, 2 pi j / nlon_out): psi_p(r, gamma) of the output point seen from the input point rotated to the pole,
  the formulas above with the centre at the input point.  Default ``theta_cutoff = (nr + 1) pi / (nlat_in - 1)``:
  the coarse grid sets the footprint.
* filter tensor: PsiT[p, k', k, D] = psi_p q'_k' with the output point at longitude 2 pi D / nlon_out relative to
  the centre, only where psi_p > 0.
* operator: y[n, k, j] = sum_{p, k', j'} PsiT[p, k', k, (j - s j') mod nlon_out] z[n, p, k', j'] (+ bias).  With
  ``normalize`` every output point is divided by its own sum A_{k, rho} = sum_{p, k', j'} PsiT, which depends on k
  and the phase rho = j mod s only: z = 1 gives y = 1 (upsampling preserves constants); a point with A = 0 stays 0.
* layer: z[b, o, p, k', j'] = sum_c W[o, c, p] x[b, c, k', j'], out[b, o] = disco_t(z)[b, o] + bias[o], W
  ``[Cout, Cin, K]``.
* table (``disco_transpose_tables``, the ``disco_t`` op, ``csrc/spectral/disco_t.hip``): a gather CSR over rows
  r = k s + rho, idx[e] = (k'_e K + p_e) nlon_in + d_e sorted within a row,
  y[n, k, s t + rho] = sum_{e in row r} val[e] z[n, p_e, k'_e, (d_e + t) mod nlon_in], 0 <= t < nlon_in; the entry of
  PsiT with D = s m + rho lands in row k s + rho with d = (nlon_in - m) mod nlon_in.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .._loader import load_plugins
from .sht import GRIDS, colatitudes

__all__ = ["disco_tables", "disco_table_holder", "disco", "kernel_size", "default_cutoff", "disco_transpose_tables",
           "disco_csr_transpose", "disco_transpose_table_holder", "disco_transpose"]

KernelShape = Union[int, Sequence[int]]


def _ops():
    load_plugins()
    return torch.ops.amd_dft


def _kernel_shape(kernel_shape: KernelShape) -> Tuple[int, int]:
    """(nr, nphi); nphi = 0: isotropic."""
    if isinstance(kernel_shape, (int, np.integer)):
        nr, nphi = int(kernel_shape), 0
    else:
        ks = tuple(int(v) for v in kernel_shape)
        if len(ks) == 1:
            nr, nphi = ks[0], 0
        elif len(ks) == 2:
            nr, nphi = ks
            if nphi < 1:
                raise ValueError(f"kernel_shape = (nr, nphi) needs nphi >= 1, got {ks}")
        else:
            raise ValueError(f"kernel_shape must be nr or (nr, nphi), got {kernel_shape!r}")
    if nr < 1:
        raise ValueError(f"kernel_shape needs nr >= 1, got {kernel_shape!r}")
    return nr, nphi


def kernel_size(kernel_shape: KernelShape) -> int:
    """K: nr for an isotropic basis, 1 + (nr - 1) nphi for an anisotropic one."""
    nr, nphi = _kernel_shape(kernel_shape)
    return nr if nphi == 0 else 1 + (nr - 1) * nphi


def default_cutoff(kernel_shape: KernelShape, nlat_out: int) -> float:
    nr, _ = _kernel_shape(kernel_shape)
    if nlat_out < 2:
        raise ValueError("the default theta_cutoff needs nlat_out >= 2")
    return (nr + 1) * math.pi / (nlat_out - 1)


def _basis(r: np.ndarray, gamma: np.ndarray, nr: int, nphi: int, cutoff: float):
    """psi_p at (r, gamma), p = 0 .. K - 1, as a list of arrays of r's shape."""
    dr = cutoff / nr
    # r < cutoff spelled out: at r == cutoff the last hat rounds to 1e-16, not 0
    hats = [np.where(r < cutoff, np.maximum(0.0, 1.0 - np.abs(r - i * dr) / dr), 0.0) for i in range(nr)]
    if nphi == 0:
        return hats
    out = [hats[0]]
    dphi = 2.0 * np.pi / nphi
    for i in range(1, nr):
        for a in range(nphi):
            d = np.abs(gamma - a * dphi)
            d = np.minimum(d, 2.0 * np.pi - d)
            out.append(hats[i] * np.maximum(0.0, 1.0 - d / dphi))
    return out


def disco_tables(in_shape: Tuple[int, int], out_shape: Tuple[int, int], kernel_shape: KernelShape,
                 grid_in: str = "equiangular", grid_out: str = "equiangular", theta_cutoff: Optional[float] = None,
                 normalize: bool = True, dtype=np.float32):
    """The filter tensor in CSR over rows p * nlat_out + k', built in float64 numpy:

    ``row_ptr`` int32 [K nlat_out + 1], ``idx`` int32 [nnz] = k nlon_in + d sorted within a row, ``val`` [nnz]
    float32 (``dtype=np.float64``: the unrounded values, what the fp64 definition and the CPU op's fp64 form read).
    Raises ``ValueError`` for a grid outside ``GRIDS``, ``nlon_in % nlon_out != 0`` and a bad ``kernel_shape``, and
    ``OverflowError`` where ``nlat_in * nlon_in`` or nnz does not fit int32."""
    return _filter_csr(in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize, dtype, True)


def _filter_csr(in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize, dtype, quad: bool):
    """The filter evaluated at every input point about every output latitude, as ``disco_tables`` returns it.
    ``quad=False`` (the transposed tables, which weight by the centre's grid): psi_p alone, without q_k."""
    nlat_in, nlon_in = (int(v) for v in in_shape)
    nlat_out, nlon_out = (int(v) for v in out_shape)
    for g in (grid_in, grid_out):
        if g not in GRIDS:
            raise ValueError(f"grid must be one of {GRIDS}, got {g!r}")
    if nlat_in < 1 or nlon_in < 1 or nlat_out < 1 or nlon_out < 1 or nlon_in % nlon_out != 0:
        raise ValueError(f"nlon_in ({nlon_in}) must be a positive multiple of nlon_out ({nlon_out})")
    if nlat_in * nlon_in >= 2 ** 31:
        raise OverflowError(f"the input grid {nlat_in} x {nlon_in} does not fit int32 indices")
    if dtype not in (np.float32, np.float64):
        raise TypeError("disco_tables: dtype must be np.float32 or np.float64")
    nr, nphi = _kernel_shape(kernel_shape)
    K = kernel_size(kernel_shape)
    cutoff = float(theta_cutoff) if theta_cutoff is not None else default_cutoff(kernel_shape, nlat_out)
    if not cutoff > 0.0:
        raise ValueError(f"theta_cutoff must be positive, got {cutoff}")
    th_in, w_in = colatitudes(nlat_in, grid_in)
    th_out, _ = colatitudes(nlat_out, grid_out)
    q = w_in * (2.0 * np.pi / nlon_in) if quad else np.ones_like(w_in)
    phi = 2.0 * np.pi * np.arange(nlon_in, dtype=np.float64) / nlon_in
    cphi, sphi = np.cos(phi)[None, :], np.sin(phi)[None, :]
    rows_idx = [[None] * nlat_out for _ in range(K)]
    rows_val = [[None] * nlat_out for _ in range(K)]
    for kp in range(nlat_out):
        tp = th_out[kp]
        # r >= |theta - theta'|: only these input rows can lie inside the cutoff
        ks = np.nonzero(np.abs(th_in - tp) < cutoff)[0]
        ct, st = np.cos(th_in[ks])[:, None], np.sin(th_in[ks])[:, None]
        z = ct * math.cos(tp) + st * math.sin(tp) * cphi
        r = np.arccos(np.clip(z, -1.0, 1.0))
        X = math.cos(tp) * st * cphi - math.sin(tp) * ct
        Y = st * sphi
        gamma = np.mod(np.arctan2(Y, X), 2.0 * np.pi)
        psis = _basis(r, gamma, nr, nphi, cutoff)
        total = 0.0
        for p, psi in enumerate(psis):
            a, d = np.nonzero(psi > 0.0)  # row-major: sorted by (k, d)
            v = psi[a, d] * q[ks[a]]
            total += float(v.sum())
            rows_idx[p][kp] = ks[a].astype(np.int64) * nlon_in + d
            rows_val[p][kp] = v
        if normalize and total > 0.0:
            for p in range(K):
                rows_val[p][kp] = rows_val[p][kp] / total
    counts = np.array([len(rows_idx[p][kp]) for p in range(K) for kp in range(nlat_out)], dtype=np.int64)
    nnz = int(counts.sum())
    if nnz >= 2 ** 31:
        raise OverflowError(f"the filter tensor has {nnz} entries, which does not fit int32")
    row_ptr = np.zeros(K * nlat_out + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(counts)
    flat_i = [rows_idx[p][kp] for p in range(K) for kp in range(nlat_out)]
    flat_v = [rows_val[p][kp] for p in range(K) for kp in range(nlat_out)]
    idx = (np.concatenate(flat_i) if nnz else np.zeros(0)).astype(np.int32)
    val = (np.concatenate(flat_v) if nnz else np.zeros(0)).astype(dtype)
    return row_ptr, idx, val


class _DiscoTables:
    """One filter tensor on one device: ``row_ptr``, ``idx``, ``val`` (fp32) as the op takes them, the host copy of
    ``row_ptr`` (checked here, on the host: non-decreasing from 0 to nnz, and every idx inside the input grid), and
    K, nnz, ``nnz_max`` (the longest row)."""

    def __init__(self, in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize, device):
        rp, idx, val = disco_tables(in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize)
        self.K = kernel_size(kernel_shape)
        self.nlat_out, self.nlon_out = int(out_shape[0]), int(out_shape[1])
        self.nnz = int(idx.shape[0])
        if rp[0] != 0 or rp[-1] != self.nnz or np.any(np.diff(rp.astype(np.int64)) < 0):
            raise ValueError("disco tables: row_ptr must run from 0 to nnz without decreasing")
        if self.nnz and (idx.min() < 0 or idx.max() >= int(in_shape[0]) * int(in_shape[1])):
            raise ValueError("disco tables: idx outside the input grid")
        self.row_ptr_host = rp
        self.nnz_max = int(np.diff(rp.astype(np.int64)).max()) if len(rp) > 1 else 0
        self.row_ptr = torch.from_numpy(rp).to(device)
        self.idx = torch.from_numpy(idx).to(device)
        self.val = torch.from_numpy(val).to(device)


_CACHE: dict = {}


def disco_table_holder(in_shape, out_shape, kernel_shape, grid_in: str = "equiangular",
                       grid_out: str = "equiangular", theta_cutoff: Optional[float] = None, normalize: bool = True,
                       device="cpu") -> _DiscoTables:
    """The tables cached per (grids, basis, cutoff, normalize, device), in the style of ``sht_tables``: they live as
    long as the process, so a captured hipGraph that reads them stays valid."""
    nr, nphi = _kernel_shape(kernel_shape)
    key = (tuple(int(v) for v in in_shape), tuple(int(v) for v in out_shape), nr, nphi, grid_in, grid_out,
           None if theta_cutoff is None else float(theta_cutoff), bool(normalize), str(torch.device(device)))
    t = _CACHE.get(key)
    if t is None:
        t = _CACHE[key] = _DiscoTables(in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize,
                                       device)
    return t


def disco_csr_transpose(row_ptr, idx, val, K: int, fine_shape: Tuple[int, int], coarse_shape: Tuple[int, int]):
    """The exact adjoint of a forward-form table, re-indexed for ``disco_t``: no reweighting, no normalisation.

    In: rows ``p * nlat_coarse + k'``, ``idx = k * nlon_fine + D`` (a ``disco`` table from the fine grid to the coarse
    one).  Out: ``(row_ptr int32 [nlat_fine * s + 1], idx int32, val)`` over rows ``k * s + rho`` with
    ``idx = (k' * K + p) * nlon_coarse + d`` sorted within a row: the entry with ``D = s m + rho`` lands in row
    ``k * s + rho`` with ``d = (nlon_coarse - m) mod nlon_coarse``."""
    nlat_f, nlon_f = (int(v) for v in fine_shape)
    nlat_c, nlon_c = (int(v) for v in coarse_shape)
    K = int(K)
    if nlat_f < 1 or nlon_f < 1 or nlat_c < 1 or nlon_c < 1 or K < 1 or nlon_f % nlon_c != 0:
        raise ValueError(f"nlon_fine ({nlon_f}) must be a positive multiple of nlon_coarse ({nlon_c})")
    if K * nlat_c * nlon_c >= 2 ** 31:
        raise OverflowError(f"the input {K} x {nlat_c} x {nlon_c} does not fit int32 indices")
    s = nlon_f // nlon_c
    if nlat_f * s >= 2 ** 31 - 1:
        raise OverflowError(f"{nlat_f} x {s} table rows do not fit int32")
    rp = np.asarray(row_ptr).astype(np.int64)
    idx = np.asarray(idx).astype(np.int64)
    val = np.asarray(val)
    if rp.shape != (K * nlat_c + 1,) or idx.shape != val.shape or idx.ndim != 1:
        raise ValueError("disco_csr_transpose: row_ptr must be [K * nlat_coarse + 1], idx and val [nnz]")
    if rp[0] != 0 or rp[-1] != len(idx) or np.any(np.diff(rp) < 0):
        raise ValueError("disco_csr_transpose: row_ptr must run from 0 to nnz without decreasing")
    if len(idx) and (idx.min() < 0 or idx.max() >= nlat_f * nlon_f):
        raise ValueError("disco_csr_transpose: idx outside the fine grid")
    rows = np.repeat(np.arange(K * nlat_c, dtype=np.int64), np.diff(rp))
    p, kc = rows // nlat_c, rows % nlat_c
    k, D = idx // nlon_f, idx % nlon_f
    m, rho = D // s, D % s
    new_row = k * s + rho
    new_idx = (kc * K + p) * nlon_c + (nlon_c - m) % nlon_c
    order = np.argsort(new_row * (K * nlat_c * nlon_c) + new_idx, kind="stable")
    out_rp = np.zeros(nlat_f * s + 1, dtype=np.int32)
    out_rp[1:] = np.cumsum(np.bincount(new_row, minlength=nlat_f * s))
    return out_rp, new_idx[order].astype(np.int32), val[order]


def disco_transpose_tables(in_shape: Tuple[int, int], out_shape: Tuple[int, int], kernel_shape: KernelShape,
                           grid_in: str = "equiangular", grid_out: str = "equiangular",
                           theta_cutoff: Optional[float] = None, normalize: bool = True, dtype=np.float32):
    """The transposed (upsampling) filter tensor in the gather CSR ``disco_t`` takes, built in float64 numpy.

    Definition (same grids, local coordinates r, gamma, basis psi_p and K as the forward layer; torch-harmonics'
    ``DiscreteContinuousConvTransposeS2`` layout, NOT its normalisation): input (coarse) grid ``in_shape``, output
    (fine) grid ``out_shape``, ``nlon_out % nlon_in == 0``, ``s = nlon_out / nlon_in`` (1 allowed), input quadrature
    weight q'_k' = w'_k' 2 pi / nlon_in.  The filter is centred on the input point (theta'_k', 2 pi j' / nlon_in) and
    evaluated at the output point (theta_k, 2 pi j / nlon_out): psi_p(r, gamma) of the output point seen from the
    input point rotated to the pole (the forward formulas with the centre at the input point); default
    ``theta_cutoff = (nr + 1) pi / (nlat_in - 1)``, the coarse grid sets the footprint.
    PsiT[p, k', k, D] = psi_p q'_k' at relative longitude 2 pi D / nlon_out, only where psi_p > 0, and

        y[n, k, j] = sum_{p, k', j'} PsiT[p, k', k, (j - s j') mod nlon_out] z[n, p, k', j'] (+ bias).

    ``normalize``: every output point is divided by its own sum A_{k, rho} = sum_{p, k', j'} PsiT, which depends on
    k and the phase rho = j mod s only, so z = 1 gives y = 1; a point with A = 0 stays 0.

    Returns ``(row_ptr int32 [nlat_out * s + 1], idx int32 [nnz], val [nnz])`` over rows ``r = k * s + rho``:
    ``idx = (k' * K + p) * nlon_in + d`` sorted within a row (k'-major: the rows of one output latitude touch one
    contiguous band of input latitudes with all K basis planes), and

        y[n, k, s t + rho] = sum_{e in row r} val[e] z[n, p_e, k'_e, (d_e + t) mod nlon_in],   0 <= t < nlon_in.

    Raises like :func:`disco_tables`: ``ValueError`` for a grid outside ``GRIDS``, ``nlon_out % nlon_in != 0`` and a
    bad ``kernel_shape``, ``OverflowError`` where an index does not fit int32, ``TypeError`` for another dtype."""
    nlat_in, nlon_in = (int(v) for v in in_shape)
    nlat_out, nlon_out = (int(v) for v in out_shape)
    for g in (grid_in, grid_out):
        if g not in GRIDS:
            raise ValueError(f"grid must be one of {GRIDS}, got {g!r}")
    if nlat_in < 1 or nlon_in < 1 or nlat_out < 1 or nlon_out < 1 or nlon_out % nlon_in != 0:
        raise ValueError(f"nlon_out ({nlon_out}) must be a positive multiple of nlon_in ({nlon_in})")
    if dtype not in (np.float32, np.float64):
        raise TypeError("disco_transpose_tables: dtype must be np.float32 or np.float64")
    K = kernel_size(kernel_shape)
    if K * nlat_in * nlon_in >= 2 ** 31:
        raise OverflowError(f"the input {K} x {nlat_in} x {nlon_in} does not fit int32 indices")
    cutoff = float(theta_cutoff) if theta_cutoff is not None else default_cutoff(kernel_shape, nlat_in)
    # psi_p of every fine point about every coarse point: the forward table from the fine grid to the coarse one
    # without its quadrature weight, rows p * nlat_in + k'
    rp, idx, psi = _filter_csr(out_shape, in_shape, kernel_shape, grid_out, grid_in, cutoff, False, np.float64, False)
    _, w_in = colatitudes(nlat_in, grid_in)
    kc = np.repeat(np.arange(K * nlat_in, dtype=np.int64) % nlat_in, np.diff(rp.astype(np.int64)))
    val = psi * (w_in * (2.0 * np.pi / nlon_in))[kc]
    rp_t, idx_t, val_t = disco_csr_transpose(rp, idx, val, K, out_shape, in_shape)
    if normalize and len(val_t):
        rows = np.repeat(np.arange(len(rp_t) - 1, dtype=np.int64), np.diff(rp_t.astype(np.int64)))
        total = np.bincount(rows, weights=val_t, minlength=len(rp_t) - 1)
        val_t = val_t / np.where(total > 0.0, total, 1.0)[rows]
    return rp_t, idx_t, val_t.astype(dtype)


class _DiscoTransposeTables:
    """One transposed filter tensor on one device: ``row_ptr``, ``idx``, ``val`` (fp32) as ``disco_t`` takes them, the
    host copy of ``row_ptr`` (checked here, on the host: non-decreasing from 0 to nnz, and every idx inside
    K * nlat_in * nlon_in), and K, s, nnz, ``nnz_max`` (the longest row)."""

    def __init__(self, in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize, device):
        rp, idx, val = disco_transpose_tables(in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff,
                                              normalize)
        self.K = kernel_size(kernel_shape)
        self.nlat_out, self.nlon_out = int(out_shape[0]), int(out_shape[1])
        self.s = self.nlon_out // int(in_shape[1])
        self.nnz = int(idx.shape[0])
        if rp[0] != 0 or rp[-1] != self.nnz or np.any(np.diff(rp.astype(np.int64)) < 0):
            raise ValueError("disco_t tables: row_ptr must run from 0 to nnz without decreasing")
        if self.nnz and (idx.min() < 0 or idx.max() >= self.K * int(in_shape[0]) * int(in_shape[1])):
            raise ValueError("disco_t tables: idx outside the input grid")
        self.row_ptr_host = rp
        self.nnz_max = int(np.diff(rp.astype(np.int64)).max()) if len(rp) > 1 else 0
        self.row_ptr = torch.from_numpy(rp).to(device)
        self.idx = torch.from_numpy(idx).to(device)
        self.val = torch.from_numpy(val).to(device)


def disco_transpose_table_holder(in_shape, out_shape, kernel_shape, grid_in: str = "equiangular",
                                 grid_out: str = "equiangular", theta_cutoff: Optional[float] = None,
                                 normalize: bool = True, device="cpu") -> _DiscoTransposeTables:
    """The transposed tables cached per (grids, basis, cutoff, normalize, device), like ``disco_table_holder``."""
    nr, nphi = _kernel_shape(kernel_shape)
    key = ("t", tuple(int(v) for v in in_shape), tuple(int(v) for v in out_shape), nr, nphi, grid_in, grid_out,
           None if theta_cutoff is None else float(theta_cutoff), bool(normalize), str(torch.device(device)))
    t = _CACHE.get(key)
    if t is None:
        t = _CACHE[key] = _DiscoTransposeTables(in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff,
                                                normalize, device)
    return t


def disco_transpose(z: torch.Tensor, tables: _DiscoTransposeTables, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``z`` [..., C, K, nlat_in, nlon_in] (fp32 or bf16) -> y [..., C, nlat_out, nlon_out] of the same dtype, plus
    ``bias`` [C] (fp32): the ``disco_t`` op on a holder's tables (the hand kernel on a GPU, its ATen counterpart on
    CPU tensors)."""
    if z.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"disco_transpose: z must be float32 or bfloat16, got {z.dtype}")
    return _ops().disco_t(z, tables.row_ptr, tables.idx, tables.val, tables.nlat_out, tables.nlon_out, bias)


def disco(x: torch.Tensor, tables: _DiscoTables) -> torch.Tensor:
    """``x`` [..., nlat_in, nlon_in] (fp32 or bf16) -> y [..., K, nlat_out, nlon_out] of the same dtype: the
    ``disco`` op on a holder's tables (the hand kernel on a GPU, its ATen counterpart on CPU tensors)."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"disco: x must be float32 or bfloat16, got {x.dtype}")
    return _ops().disco(x, tables.row_ptr, tables.idx, tables.val, tables.K, tables.nlat_out, tables.nlon_out)
