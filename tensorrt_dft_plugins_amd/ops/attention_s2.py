"""Attention on the sphere: neighbourhood attention (the half-width table and the ``attention_s2`` op) and global
attention (``attention_s2_global``, at the end of this module).

Attention of every output point over the input points within a geodesic cutoff, weighted by the quadrature of the
input grid: the ``NeighborhoodAttentionS2`` layer of spherical transformers and of the attention variants of
spherical U-Nets (the layout of torch-harmonics' layer; no published weights are involved).

Definition:

* grids as in :mod:`.disco`: input ``(nlat_in, nlon_in, grid_in)``, output ``(nlat_out, nlon_out, grid_out)``, the
  colatitudes theta_k and weights w_k of :func:`.sht.colatitudes`; ``nlon_in % nlon_out == 0``,
  ``s = nlon_in / nlon_out``.
* neighbourhood: input point (k, j) is a neighbour of output point (k', j') iff the geodesic distance
  r = arccos(cos theta_k cos theta'_k' + sin theta_k sin theta'_k' cos phi) < theta_cutoff at
  phi = 2 pi (j - s j') / nlon_in: the r and the strict comparison of the DISCO filter.  r is monotone in |phi| on
  [0, pi], so the neighbours in row k are the longitudes with circular |j - s j'| <= hw[k', k].  ``hw`` int32
  [nlat_out, nlat_in] is the whole table: -1 no neighbour in that row, values at most nlon_in // 2, and
  2 hw + 1 >= nlon_in the whole row, each longitude once.  Default ``theta_cutoff = 2 pi / (nlat_out - 1)``
  (``default_cutoff(1, nlat_out)``).
* operator: q [B, heads * d, nlat_out, nlon_out], k and v [B, heads * d, nlat_in, nlon_in], head h owning the
  channels h d .. (h + 1) d - 1; with logw[k] = log w_k

      score(k, j) = scale sum_c q[b, h, c, k', j'] k[b, h, c, k, j] + logw[k]
      y[b, h, :, k', j'] = sum_{(k, j) in N(k', j')} softmax_N(score)(k, j) v[b, h, :, k, j]

  An output point with an empty neighbourhood gives 0.  The constant 2 pi / nlon_in of the quadrature cancels in
  the softmax and is left out.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .._loader import load_plugins
from .disco import _cached, default_cutoff
from .sht import GRIDS, colatitudes

__all__ = ["attention_s2_tables", "attention_s2_table_holder", "attention_s2", "attention_s2_global_tables",
           "attention_s2_global_table_holder", "attention_s2_global"]


def _ops():
    load_plugins()
    return torch.ops.amd_dft


def attention_s2_tables(in_shape: Tuple[int, int], out_shape: Tuple[int, int], grid_in: str = "equiangular",
                        grid_out: str = "equiangular", theta_cutoff: Optional[float] = None, dtype=np.float32):
    """``(hw int32 [nlat_out, nlat_in], logw [nlat_in])`` built in float64 numpy; ``logw`` is rounded to ``dtype``
    (``np.float64``: the unrounded values, what the fp64 definition reads).  Raises ``ValueError`` for a grid
    outside ``GRIDS``, ``nlon_in % nlon_out != 0`` and a cutoff that is not positive."""
    nlat_in, nlon_in = (int(v) for v in in_shape)
    nlat_out, nlon_out = (int(v) for v in out_shape)
    for g in (grid_in, grid_out):
        if g not in GRIDS:
            raise ValueError(f"grid must be one of {GRIDS}, got {g!r}")
    if nlat_in < 1 or nlon_in < 1 or nlat_out < 1 or nlon_out < 1 or nlon_in % nlon_out != 0:
        raise ValueError(f"nlon_in ({nlon_in}) must be a positive multiple of nlon_out ({nlon_out})")
    if dtype not in (np.float32, np.float64):
        raise TypeError("attention_s2_tables: dtype must be np.float32 or np.float64")
    cutoff = float(theta_cutoff) if theta_cutoff is not None else default_cutoff(1, nlat_out)
    if not cutoff > 0.0:
        raise ValueError(f"theta_cutoff must be positive, got {cutoff}")
    th_in, w_in = colatitudes(nlat_in, grid_in)
    th_out, _ = colatitudes(nlat_out, grid_out)
    # the geodesic distance at every longitude offset, as the DISCO filter evaluates it
    cphi = np.cos(2.0 * np.pi * np.arange(nlon_in, dtype=np.float64) / nlon_in)[None, None, :]
    ct, st = np.cos(th_in)[None, :, None], np.sin(th_in)[None, :, None]
    cp, sp = np.cos(th_out)[:, None, None], np.sin(th_out)[:, None, None]
    r = np.arccos(np.clip(ct * cp + st * sp * cphi, -1.0, 1.0))  # [nlat_out, nlat_in, nlon_in]
    off = np.arange(nlon_in)
    circ = np.minimum(off, nlon_in - off)[None, None, :]
    hw = np.where(r < cutoff, circ, -1).max(axis=-1).astype(np.int32)
    return hw, np.log(w_in).astype(dtype)


class _AttentionS2Tables:
    """The tables of one pair of grids on one device: ``hw`` and ``logw`` (fp32) as the op takes them, ``logw64``
    for float64 CPU tensors, and the host copy of ``hw``."""

    def __init__(self, in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize, device):
        hw, logw = attention_s2_tables(in_shape, out_shape, grid_in, grid_out, theta_cutoff, dtype=np.float64)
        self.in_shape = tuple(int(v) for v in in_shape)
        self.out_shape = tuple(int(v) for v in out_shape)
        self.hw_host = hw
        self.hw = torch.from_numpy(hw).to(device)
        self.logw64 = torch.from_numpy(logw).to(device)
        self.logw = self.logw64.float()


def attention_s2_table_holder(in_shape, out_shape, grid_in: str = "equiangular", grid_out: str = "equiangular",
                              theta_cutoff: Optional[float] = None, device="cpu") -> _AttentionS2Tables:
    """The tables cached per (grids, cutoff, device) in the cache of ``disco_table_holder``: they live as long as the
    process, so a captured hipGraph that reads them stays valid."""
    return _cached(_AttentionS2Tables, ("attn",), in_shape, out_shape, 1, grid_in, grid_out, theta_cutoff, True, device)


def attention_s2(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, tables: _AttentionS2Tables,
                 scale: Optional[float] = None, heads: int = 1) -> torch.Tensor:
    """``q`` [B, heads * d, nlat_out, nlon_out], ``k`` and ``v`` [B, heads * d, nlat_in, nlon_in], all fp32 or all
    bf16 (fp64 on CPU tensors) -> y as q: the ``attention_s2`` op on a holder's tables (the hand kernel on a GPU, the
    plain C++ definition on CPU tensors).  ``scale`` defaults to d ** -0.5.  Mixed dtypes raise ``TypeError``."""
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError(f"attention_s2: q, k and v must share one dtype, got {q.dtype}, {k.dtype} and {v.dtype}")
    if q.dtype not in (torch.float32, torch.bfloat16) and not (q.dtype == torch.float64 and q.device.type == "cpu"):
        raise TypeError(f"attention_s2: q must be float32 or bfloat16 (float64 on CPU tensors), got {q.dtype}")
    heads = int(heads)
    if heads < 1 or q.dim() != 4 or q.shape[1] % heads:
        raise ValueError(f"attention_s2: q must be [B, heads * d, nlat_out, nlon_out], got {tuple(q.shape)} with "
                         f"heads = {heads}")
    if scale is None:
        scale = float(q.shape[1] // heads) ** -0.5
    logw = tables.logw64 if q.dtype == torch.float64 else tables.logw
    return _ops().attention_s2(q, k, v, tables.hw, logw, heads, float(scale))


# ---- global attention: every output point over ALL input points, any two grids
#     score(k, j) = scale sum_c q[b, h, c, k', j'] k[b, h, c, k, j] + logw[k]
#     y[b, h, :, k', j'] = sum_{all (k, j)} softmax(score)(k, j) v[b, h, :, k, j]
# The only table is logw[k] = log w_k of the input grid; the output grid enters through q's shape alone.


def attention_s2_global_tables(in_shape: Tuple[int, int], grid_in: str = "equiangular", dtype=np.float32):
    """``logw [nlat_in]`` = log of the quadrature weights of the input grid (:func:`.sht.colatitudes`), built in
    float64 numpy and rounded to ``dtype``.  Raises ``ValueError`` for a grid outside ``GRIDS`` or an empty shape."""
    nlat_in, nlon_in = (int(v) for v in in_shape)
    if grid_in not in GRIDS:
        raise ValueError(f"grid must be one of {GRIDS}, got {grid_in!r}")
    if nlat_in < 1 or nlon_in < 1:
        raise ValueError(f"in_shape must be positive, got {tuple(in_shape)}")
    if dtype not in (np.float32, np.float64):
        raise TypeError("attention_s2_global_tables: dtype must be np.float32 or np.float64")
    return np.log(colatitudes(nlat_in, grid_in)[1]).astype(dtype)


class _AttentionS2GlobalTables:
    """``logw`` (fp32) of one input grid on one device as the op takes it, and ``logw64`` for float64 CPU tensors."""

    def __init__(self, in_shape, out_shape, kernel_shape, grid_in, grid_out, theta_cutoff, normalize, device):
        self.in_shape = tuple(int(v) for v in in_shape)
        self.logw64 = torch.from_numpy(attention_s2_global_tables(in_shape, grid_in, dtype=np.float64)).to(device)
        self.logw = self.logw64.float()


def attention_s2_global_table_holder(in_shape, grid_in: str = "equiangular",
                                     device="cpu") -> _AttentionS2GlobalTables:
    """The table cached per (input grid, device) in the cache of ``disco_table_holder``."""
    return _cached(_AttentionS2GlobalTables, ("attn_global",), in_shape, in_shape, 1, grid_in, grid_in, None, True,
                   device)


def attention_s2_global(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, tables: _AttentionS2GlobalTables,
                        scale: Optional[float] = None, heads: int = 1) -> torch.Tensor:
    """``q`` [B, heads * d, nlat_out, nlon_out], ``k`` and ``v`` [B, heads * d, nlat_in, nlon_in], all fp32 or all
    bf16 (fp64 on CPU tensors) -> y as q: the ``attention_s2_global`` op (the dense MFMA kernel on a GPU, d <= 128;
    the plain C++ definition on CPU tensors).  ``scale`` defaults to d ** -0.5.  Mixed dtypes raise ``TypeError``."""
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError(f"attention_s2_global: q, k and v must share one dtype, got {q.dtype}, {k.dtype} and "
                        f"{v.dtype}")
    if q.dtype not in (torch.float32, torch.bfloat16) and not (q.dtype == torch.float64 and q.device.type == "cpu"):
        raise TypeError(f"attention_s2_global: q must be float32 or bfloat16 (float64 on CPU tensors), got {q.dtype}")
    heads = int(heads)
    if heads < 1 or q.dim() != 4 or q.shape[1] % heads:
        raise ValueError(f"attention_s2_global: q must be [B, heads * d, nlat_out, nlon_out], got {tuple(q.shape)} "
                         f"with heads = {heads}")
    if scale is None:
        scale = float(q.shape[1] // heads) ** -0.5
    logw = tables.logw64 if q.dtype == torch.float64 else tables.logw
    return _ops().attention_s2_global(q, k, v, logw, heads, float(scale))
