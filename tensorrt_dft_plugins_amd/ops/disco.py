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
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .._loader import load_plugins
from .sht import GRIDS, colatitudes

__all__ = ["disco_tables", "disco_table_holder", "disco", "kernel_size", "default_cutoff"]

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
    q = w_in * (2.0 * np.pi / nlon_in)
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


def disco(x: torch.Tensor, tables: _DiscoTables) -> torch.Tensor:
    """``x`` [..., nlat_in, nlon_in] (fp32 or bf16) -> y [..., K, nlat_out, nlon_out] of the same dtype: the
    ``disco`` op on a holder's tables (the hand kernel on a GPU, its ATen counterpart on CPU tensors)."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"disco: x must be float32 or bfloat16, got {x.dtype}")
    return _ops().disco(x, tables.row_ptr, tables.idx, tables.val, tables.K, tables.nlat_out, tables.nlon_out)
