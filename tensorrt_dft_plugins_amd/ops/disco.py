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
* table (``disco_transpose_tables``, the ``disco_t`` op, ``csrc/spectral/disco.hip`` too): a gather CSR over rows
  r = k s + rho, idx[e] = (k'_e K + p_e) nlon_in + d_e sorted within a row,
  y[n, k, s t + rho] = sum_{e in row r} val[e] z[n, p_e, k'_e, (d_e + t) mod nlon_in], 0 <= t < nlon_in; the entry of
  PsiT with D = s m + rho lands in row k s + rho with d = (nlon_in - m) mod nlon_in.

The longitude-Fourier route of the forward convolution (``disco_spectral``, ``csrc/spectral/disco_spectral.hip``; opt
in, the gather route above is the default).  Every row is a circular correlation along longitude, so with
Mi = nlon_in // 2 + 1, Mo = nlon_out // 2 + 1:

* X[k, mu] = sum_j x[k, j] e^{-2 pi i mu j / nlon_in}, the unnormalised ``r2c``, stored for mu < Mi and completed as
  X[k, mu] = conj(X[k, nlon_in - mu]) above;
* G[p, k', k, mu] = conj(sum_d Psi[p, k', k, d] e^{-2 pi i mu d / nlon_in}), 0 <= mu < nlon_in (real for an
  isotropic basis, complex in general);
* Yh[p, k', m'] = (1 / s) sum_{r < s} sum_k G[p, k', k, m' + r nlon_out] X[k, m' + r nlon_out], 0 <= m' < Mo: the
  fold of s input modes onto one output mode is the subsampling to the coarse grid;
* y[p, k', :] = irfft(Yh[p, k', :], n = nlon_out), backward norm.

Packed table (``disco_spectral_tables``): output latitudes in groups of R consecutive k' (R the largest of 8, 4, 2, 1
with R K <= 16, the last group ragged with zero rows); group g touches the input latitudes lo[g] .. hi[g], U the
tallest such band; ``T[g, m', row, kappa]`` with row = (k' - g R) K + p < 16 and kappa = 2 (r U + k - lo[g]) + c holding
Re G / s (c = 0) and Im G / s (c = 1) at mu = m' + r nlon_out, zero-padded to KD = ceil32(2 s U).

The longitude-Fourier route of the transposed convolution (``disco_spectral_transpose``, the ``disco_spectral_t`` op,
the same kernel template; opt in).  y is the circular convolution of PsiT[p, k', k, .] with z upsampled by zeros, and
the DFT of a zero-upsampled signal is the periodic extension of the coarse spectrum, so with s = nlon_out / nlon_in:

* Z[p, k', nu] the unnormalised ``r2c`` of z, stored for nu < Mi, Z[nu] = conj(Z[nlon_in - nu]) above;
* H[p, k', k, mu] = sum_D PsiT[p, k', k, D] e^{-2 pi i mu D / nlon_out} (a convolution: no conjugate); the CSR entry
  of row k s + rho with idx = (k' K + p) nlon_in + d sits at D = s ((nlon_in - d) mod nlon_in) + rho;
* Yh[k, mu] = sum_{p, k'} H[p, k', k, mu] Z[p, k', mu mod nlon_in], 0 <= mu < Mo: no fold and no 1 / s, each coarse
  mode feeds up to s fine modes; the bias adds nlon_out bias[c] to Re Yh[k, 0];
* y[k, :] = irfft(Yh[k, :], n = nlon_out), backward norm.

Packed table (``disco_spectral_transpose_tables``): groups of 16 consecutive OUTPUT latitudes (the output has no
basis index; the K basis planes sit in the contraction, so any K works), group g reads the coarse latitudes
lo[g] .. lo[g] + U - 1; ``T[g, mu, k - 16 g, kappa]`` with kappa = 2 (p U + k' - lo[g]) + c holding Re H (c = 0) and
Im H (c = 1), zero-padded to KD = ceil32(2 K U).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .._loader import load_plugins
from .sht import GRIDS, colatitudes

__all__ = ["disco_tables", "disco_table_holder", "disco", "kernel_size", "default_cutoff", "disco_transpose_tables",
           "disco_csr_transpose", "disco_transpose_table_holder", "disco_transpose", "disco_spectral_tables",
           "disco_spectral_table_holder", "disco_spectral", "disco_spectral_group", "disco_spectral_transpose_tables",
           "disco_spectral_transpose_table_holder", "disco_spectral_transpose"]

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


class _Tables:
    """One filter tensor on one device: ``row_ptr``, ``idx``, ``val`` (fp32) as the op takes them, the host copy of
    ``row_ptr`` (checked here, on the host: non-decreasing from 0 to nnz, and every idx inside the input), and
    K, nnz, ``nnz_max`` (the longest row).  A direction names its ``_build``-er, its ``_op`` for the error texts and
    whether an idx runs over the ``_basis_planes`` too."""

    def __init__(self, in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize, device):
        rp, idx, val = self._build(in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize)
        self.K = kernel_size(kernel_shape)
        self.nlat_out, self.nlon_out = int(out_shape[0]), int(out_shape[1])
        self.nnz = int(idx.shape[0])
        if rp[0] != 0 or rp[-1] != self.nnz or np.any(np.diff(rp.astype(np.int64)) < 0):
            raise ValueError(f"{self._op} tables: row_ptr must run from 0 to nnz without decreasing")
        bound = (self.K if self._basis_planes else 1) * int(in_shape[0]) * int(in_shape[1])
        if self.nnz and (idx.min() < 0 or idx.max() >= bound):
            raise ValueError(f"{self._op} tables: idx outside the input grid")
        self.row_ptr_host = rp
        self.nnz_max = int(np.diff(rp.astype(np.int64)).max()) if len(rp) > 1 else 0
        self.row_ptr = torch.from_numpy(rp).to(device)
        self.idx = torch.from_numpy(idx).to(device)
        self.val = torch.from_numpy(val).to(device)


class _DiscoTables(_Tables):
    """The forward filter tensor as ``disco`` takes it: every idx inside the input grid."""
    _build, _op, _basis_planes = staticmethod(disco_tables), "disco", False


_CACHE: dict = {}


def _cached(cls, tag, in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize, device):
    nr, nphi = _kernel_shape(kernel_shape)
    key = tag + (tuple(int(v) for v in in_shape), tuple(int(v) for v in out_shape), nr, nphi, grid_in, grid_out,
                 None if theta_cutoff is None else float(theta_cutoff), bool(normalize), str(torch.device(device)))
    t = _CACHE.get(key)
    if t is None:
        t = _CACHE[key] = cls(in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize, device)
    return t


def disco_table_holder(in_shape, out_shape, kernel_shape, grid_in: str = "equiangular",
                       grid_out: str = "equiangular", theta_cutoff: Optional[float] = None, normalize: bool = True,
                       device="cpu") -> _DiscoTables:
    """The tables cached per (grids, basis, cutoff, normalize, device), in the style of ``sht_tables``: they live as
    long as the process, so a captured hipGraph that reads them stays valid."""
    return _cached(_DiscoTables, (), in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize,
                   device)


def disco_spectral_group(K: int) -> int:
    """R: output latitudes per group of the spectral table, the largest of 8, 4, 2, 1 with R K <= 16."""
    if not 1 <= int(K) <= 16:
        raise ValueError(f"the longitude-Fourier route takes 1 <= K <= 16 basis functions, got {K}")
    return next(r for r in (8, 4, 2, 1) if r * int(K) <= 16)


def disco_spectral_tables(in_shape: Tuple[int, int], out_shape: Tuple[int, int], kernel_shape: KernelShape,
                          grid_in: str = "equiangular", grid_out: str = "equiangular",
                          theta_cutoff: Optional[float] = None, normalize: bool = True, dtype=np.float32):
    """The packed table of the longitude-Fourier route, built in float64 numpy from the CSR of ``disco_tables``, one
    group of output latitudes at a time (the dense Psi of the whole grid is never held).

    Returns ``(T [G, Mo, 16, KD] of dtype, lo int32 [G], U)``: the layout of the module docstring.  T carries the
    1 / s of the fold and nothing else: the remaining factor of the inverse transform, 1 / nlon_out, is the ``scale``
    argument of the one ``c2r`` call that finishes the job (``disco_spectral``).  A group without entries has
    lo = 0 and an all-zero table.  Raises like ``disco_tables``, and ``ValueError`` for K > 16."""
    if dtype not in (np.float32, np.float64):
        raise TypeError("disco_spectral_tables: dtype must be np.float32 or np.float64")
    rp, idx, val = disco_tables(in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize,
                                dtype=np.float64)
    nlat_in, nlon_in = (int(v) for v in in_shape)
    nlat_out, nlon_out = (int(v) for v in out_shape)
    K = kernel_size(kernel_shape)
    R = disco_spectral_group(K)
    G, s, Mo = -(-nlat_out // R), nlon_in // nlon_out, nlon_out // 2 + 1
    rp = rp.astype(np.int64)
    krow, d = idx.astype(np.int64) // nlon_in, idx.astype(np.int64) % nlon_in

    def entries(g):  # (row of the tile, k, d, value) of every entry of group g
        out = []
        for kl in range(min(R, nlat_out - g * R)):
            for p in range(K):
                a, b = rp[p * nlat_out + g * R + kl], rp[p * nlat_out + g * R + kl + 1]
                out.append((np.full(b - a, kl * K + p), krow[a:b], d[a:b], val[a:b]))
        return tuple(np.concatenate(c) for c in zip(*out))

    lo = np.zeros(G, dtype=np.int32)
    U = 1
    for g in range(G):
        _, k, _, _ = entries(g)
        if len(k):
            lo[g] = k.min()
            U = max(U, int(k.max()) - int(k.min()) + 1)
    KD = -(-2 * s * U // 32) * 32
    T = np.zeros((G, Mo, 16, KD), dtype=dtype)
    mu = np.arange(Mo)[None, :] + nlon_out * np.arange(s)[:, None]  # [s, Mo]
    for g in range(G):
        row, k, dd, v = entries(g)
        psi = np.zeros((16, U, nlon_in))
        psi[row, k - lo[g], dd] = v
        Gs = np.conj(np.fft.fft(psi, axis=-1))[:, :, mu] / s     # [16, U, s, Mo]
        Gs = Gs.transpose(3, 0, 2, 1).reshape(Mo, 16, s * U)     # j = r U + dk
        T[g, :, :, 0:2 * s * U:2] = Gs.real
        T[g, :, :, 1:2 * s * U:2] = Gs.imag
    return T, lo, U


class _DiscoSpectralTables:
    """The packed table on one device as ``disco_spectral`` takes it: ``table`` bf16 [2, G, Mo, 16, KD], the fp32
    values split once, on the host, into the planes hi = bf16(T) and lo = bf16(T - hi) (``table_bf16``: the hi plane
    alone, [1, G, Mo, 16, KD], what a bf16 call takes), ``lo`` int32 [G], and K, R, U, KD, s, Mo, ``table_bytes``."""

    def __init__(self, in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize, device):
        T, lo, U = disco_spectral_tables(in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize)
        self.K = kernel_size(kernel_shape)
        self.R, self.U, self.KD = disco_spectral_group(self.K), int(U), int(T.shape[-1])
        self.nlat_out, self.nlon_out = int(out_shape[0]), int(out_shape[1])
        self.nlon_in = int(in_shape[1])
        self.s, self.Mo = self.nlon_in // self.nlon_out, self.nlon_out // 2 + 1
        t32 = torch.from_numpy(T)
        hi = t32.to(torch.bfloat16)
        self.table = torch.stack([hi, (t32 - hi.float()).to(torch.bfloat16)]).to(device)
        self.table_bf16 = self.table[:1]
        self.table_bytes = self.table.numel() * 2
        self.lo = torch.from_numpy(lo).to(device)


def disco_spectral_table_holder(in_shape, out_shape, kernel_shape, grid_in: str = "equiangular",
                                grid_out: str = "equiangular", theta_cutoff: Optional[float] = None,
                                normalize: bool = True, device="cpu") -> _DiscoSpectralTables:
    """The spectral tables cached per (grids, basis, cutoff, normalize, device), like ``disco_table_holder``; one
    table serves every layer on the same grids."""
    return _cached(_DiscoSpectralTables, ("spectral",), in_shape, out_shape, kernel_shape, grid_in, grid_out,
                   theta_cutoff, normalize, device)


def disco_spectral(x: torch.Tensor, tables: _DiscoSpectralTables) -> torch.Tensor:
    """``x`` [..., nlat_in, nlon_in] (fp32 or bf16) -> y [..., K, nlat_out, nlon_out] of the same dtype, the shape and
    meaning of ``disco(x, tables)`` by the longitude-Fourier route: ``r2c`` along longitude (all modes), the
    ``disco_spectral`` op, ``c2r`` to nlon_out with scale 1 / nlon_out."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"disco_spectral: x must be float32 or bfloat16, got {x.dtype}")
    if x.dim() < 2 or int(x.shape[-1]) != tables.nlon_in:
        raise ValueError(f"disco_spectral: x must be [..., nlat_in, {tables.nlon_in}], got {tuple(x.shape)}")
    ops = _ops()
    xh = ops.r2c(x, [x.dim() - 1], 1.0, [], x.dtype)  # [..., nlat_in, Mi, 2]
    table = tables.table_bf16 if x.dtype == torch.bfloat16 else tables.table
    yh = ops.disco_spectral(xh, table, tables.lo, tables.K, tables.U, tables.nlat_out, tables.nlon_in, tables.nlon_out)
    return ops.c2r(yh, [yh.dim() - 2], [tables.nlon_out], 1.0 / tables.nlon_out, [], x.dtype)


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


class _DiscoTransposeTables(_Tables):
    """The transposed filter tensor as ``disco_t`` takes it: every idx inside K * nlat_in * nlon_in; also s."""
    _build, _op, _basis_planes = staticmethod(disco_transpose_tables), "disco_t", True

    def __init__(self, in_shape, out_shape, *args):
        super().__init__(in_shape, out_shape, *args)
        self.s = self.nlon_out // int(in_shape[1])


def disco_transpose_table_holder(in_shape, out_shape, kernel_shape, grid_in: str = "equiangular",
                                 grid_out: str = "equiangular", theta_cutoff: Optional[float] = None,
                                 normalize: bool = True, device="cpu") -> _DiscoTransposeTables:
    """The transposed tables cached per (grids, basis, cutoff, normalize, device), like ``disco_table_holder``."""
    return _cached(_DiscoTransposeTables, ("t",), in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff,
                   normalize, device)


def disco_transpose(z: torch.Tensor, tables: _DiscoTransposeTables, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``z`` [..., C, K, nlat_in, nlon_in] (fp32 or bf16) -> y [..., C, nlat_out, nlon_out] of the same dtype, plus
    ``bias`` [C] (fp32): the ``disco_t`` op on a holder's tables (the hand kernel on a GPU, its ATen counterpart on
    CPU tensors)."""
    if z.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"disco_transpose: z must be float32 or bfloat16, got {z.dtype}")
    return _ops().disco_t(z, tables.row_ptr, tables.idx, tables.val, tables.nlat_out, tables.nlon_out, bias)


def disco_spectral_transpose_tables(in_shape: Tuple[int, int], out_shape: Tuple[int, int], kernel_shape: KernelShape,
                                    grid_in: str = "equiangular", grid_out: str = "equiangular",
                                    theta_cutoff: Optional[float] = None, normalize: bool = True, dtype=np.float32):
    """The packed table of the transposed longitude-Fourier route, built in float64 numpy from the CSR of
    ``disco_transpose_tables``, one group of 16 output latitudes at a time (the dense PsiT of the whole grid is never
    held).

    Returns ``(T [G, Mo, 16, KD] of dtype, lo int32 [G], U)``: the layout of the module docstring.  The per-phase
    normalisation is in the CSR's values already and T carries nothing else: 1 / nlon_out is the ``scale`` of the one
    ``c2r`` call that finishes the job (``disco_spectral_transpose``).  A group without entries has lo = 0 and an
    all-zero table.  Raises like ``disco_transpose_tables``; any K >= 1."""
    if dtype not in (np.float32, np.float64):
        raise TypeError("disco_spectral_transpose_tables: dtype must be np.float32 or np.float64")
    rp, idx, val = disco_transpose_tables(in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize,
                                          dtype=np.float64)
    nlon_in = int(in_shape[1])
    nlat_out, nlon_out = (int(v) for v in out_shape)
    K = kernel_size(kernel_shape)
    G, s, Mo = -(-nlat_out // 16), nlon_out // nlon_in, nlon_out // 2 + 1
    rp, idx = rp.astype(np.int64), idx.astype(np.int64)
    erow = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))  # k s + rho of every entry
    q, d = idx // nlon_in, idx % nlon_in
    kin, p = q // K, q % K
    big_d = s * ((nlon_in - d) % nlon_in) + erow % s  # D, the relative longitude on the fine grid
    spans = [slice(rp[16 * g * s], rp[min(16 * g + 16, nlat_out) * s]) for g in range(G)]
    lo = np.zeros(G, dtype=np.int32)
    U = 1
    for g, e in enumerate(spans):
        if e.stop > e.start:
            lo[g] = kin[e].min()
            U = max(U, int(kin[e].max()) - int(lo[g]) + 1)
    KD = -(-2 * K * U // 32) * 32
    T = np.zeros((G, Mo, 16, KD), dtype=dtype)
    for g, e in enumerate(spans):
        psi = np.zeros((16, K * U, nlon_out))
        psi[erow[e] // s - 16 * g, p[e] * U + kin[e] - lo[g], big_d[e]] = val[e]
        H = np.fft.rfft(psi, axis=-1).transpose(2, 0, 1)  # [Mo, 16, j = p U + dk]
        T[g, :, :, 0:2 * K * U:2] = H.real
        T[g, :, :, 1:2 * K * U:2] = H.imag
    return T, lo, U


class _DiscoSpectralTransposeTables:
    """The packed transposed table on one device as ``disco_spectral_t`` takes it: ``table`` bf16 [2, G, Mo, 16, KD],
    the fp32 values split once, on the host, into the planes hi = bf16(T) and lo = bf16(T - hi) (``table_bf16``: the
    hi plane alone, [1, G, Mo, 16, KD], what a bf16 call takes), ``lo`` int32 [G], and K, U, KD, s, Mo,
    ``table_bytes``."""

    def __init__(self, in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize, device):
        T, lo, U = disco_spectral_transpose_tables(in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff,
                                                   normalize)
        self.K, self.U, self.KD = kernel_size(kernel_shape), int(U), int(T.shape[-1])
        self.nlat_out, self.nlon_out = int(out_shape[0]), int(out_shape[1])
        self.nlat_in, self.nlon_in = int(in_shape[0]), int(in_shape[1])
        self.s, self.Mo = self.nlon_out // self.nlon_in, self.nlon_out // 2 + 1
        t32 = torch.from_numpy(T)
        hi = t32.to(torch.bfloat16)
        self.table = torch.stack([hi, (t32 - hi.float()).to(torch.bfloat16)]).to(device)
        self.table_bf16 = self.table[:1]
        self.table_bytes = self.table.numel() * 2
        self.lo = torch.from_numpy(lo).to(device)


def disco_spectral_transpose_table_holder(in_shape, out_shape, kernel_shape, grid_in: str = "equiangular",
                                          grid_out: str = "equiangular", theta_cutoff: Optional[float] = None,
                                          normalize: bool = True, device="cpu") -> _DiscoSpectralTransposeTables:
    """The transposed spectral tables cached per (grids, basis, cutoff, normalize, device), like
    ``disco_spectral_table_holder``."""
    return _cached(_DiscoSpectralTransposeTables, ("spectral_t",), in_shape, out_shape, kernel_shape, grid_in, grid_out,
                   theta_cutoff, normalize, device)


def disco_spectral_transpose(z: torch.Tensor, tables: _DiscoSpectralTransposeTables,
                             bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``z`` [..., C, K, nlat_in, nlon_in] (fp32 or bf16) -> y [..., C, nlat_out, nlon_out] of the same dtype, plus
    ``bias`` [C] (fp32): the shape and meaning of ``disco_transpose(z, tables, bias)`` by the longitude-Fourier
    route: ``r2c`` along longitude (all modes), the ``disco_spectral_t`` op (which adds the bias, at mode 0), ``c2r``
    to nlon_out with scale 1 / nlon_out."""
    if z.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"disco_spectral_transpose: z must be float32 or bfloat16, got {z.dtype}")
    if z.dim() < 4 or tuple(z.shape[-3:]) != (tables.K, tables.nlat_in, tables.nlon_in):
        raise ValueError(f"disco_spectral_transpose: z must be [..., C, {tables.K}, {tables.nlat_in}, "
                         f"{tables.nlon_in}], got {tuple(z.shape)}")
    ops = _ops()
    zh = ops.r2c(z, [z.dim() - 1], 1.0, [], z.dtype)  # [..., C, K, nlat_in, Mi, 2]
    table = tables.table_bf16 if z.dtype == torch.bfloat16 else tables.table
    yh = ops.disco_spectral_t(zh, table, tables.lo, tables.K, tables.U, tables.nlat_out, tables.nlon_in,
                              tables.nlon_out, bias)
    return ops.c2r(yh, [yh.dim() - 2], [tables.nlon_out], 1.0 / tables.nlon_out, [], z.dtype)


def disco(x: torch.Tensor, tables: _DiscoTables) -> torch.Tensor:
    """``x`` [..., nlat_in, nlon_in] (fp32 or bf16) -> y [..., K, nlat_out, nlon_out] of the same dtype: the
    ``disco`` op on a holder's tables (the hand kernel on a GPU, its ATen counterpart on CPU tensors)."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"disco: x must be float32 or bfloat16, got {x.dtype}")
    return _ops().disco(x, tables.row_ptr, tables.idx, tables.val, tables.K, tables.nlat_out, tables.nlon_out)
