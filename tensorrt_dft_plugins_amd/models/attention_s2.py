"""``NeighborhoodAttentionS2``: multi-head attention on the sphere restricted to a geodesic neighbourhood and weighted
by the quadrature of the input grid, the attention layer of spherical transformers and of the attention variants of
spherical U-Nets (definition: :mod:`..ops.attention_s2`).

Backends: ``"amd"`` (the default): three ``fno_pointwise`` projections, the ``attention_s2`` op
(``csrc/spectral/attention_s2.hip`` on a GPU, the plain C++ definition on CPU tensors) and one ``fno_pointwise``
output projection, in fp32 or bf16.  ``"torch"``: the definition and the numerics oracle, a masked softmax per output
latitude in eager torch -- what a user writes without the op; it follows the input's precision (fp64 in, fp64 out; a
bf16 input is computed in fp32 and rounded once).

The projection weights are ``[C, C]`` (``[out_chans, C]`` for the output), torch-harmonics' layer layout; published
weights are not involved.  Out of scope: autograd, dropout, a fused q/k/v projection.

``AttentionS2``: the same layer over ALL input points (global attention, the coarse levels of a spherical
transformer and the cross-attention between two grids): no cutoff, any two grids.  Its amd backend runs the
``attention_s2_global`` op (``csrc/spectral/attention_s2_global.hip``).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from ..ops import attention_s2 as A

__all__ = ["NeighborhoodAttentionS2", "AttentionS2"]


class NeighborhoodAttentionS2(nn.Module):
    """``forward(query, key=None, value=None)``: ``query`` [B, in_chans, nlat_out, nlon_out] on the output grid,
    ``key`` and ``value`` [B, in_chans, nlat_in, nlon_in] on the input grid (``key`` defaults to ``query`` where the
    grids are equal, ``value`` to ``key``) -> [B, out_chans, nlat_out, nlon_out]."""

    def __init__(self, in_chans: int, in_shape: Tuple[int, int], out_shape: Tuple[int, int], num_heads: int = 1,
                 grid_in: str = "equiangular", grid_out: str = "equiangular", theta_cutoff: Optional[float] = None,
                 bias: bool = True, out_chans: Optional[int] = None, backend: str = "amd"):
        super().__init__()
        if backend not in ("torch", "amd"):
            raise ValueError(f"backend must be 'torch' or 'amd', got {backend!r}")
        self.in_chans = int(in_chans)
        self.out_chans = int(out_chans) if out_chans is not None else self.in_chans
        self.num_heads = int(num_heads)
        if self.num_heads < 1 or self.in_chans % self.num_heads:
            raise ValueError(f"in_chans ({self.in_chans}) must be a multiple of num_heads ({self.num_heads})")
        self.in_shape = tuple(int(v) for v in in_shape)
        self.out_shape = tuple(int(v) for v in out_shape)
        self.grid_in, self.grid_out = grid_in, grid_out
        self.theta_cutoff = (float(theta_cutoff) if theta_cutoff is not None
                             else A.default_cutoff(1, self.out_shape[0]))
        self.backend = backend
        # d ** -0.5 as fp32: the value the kernel takes and an exported graph's float attribute carries
        self.scale = float(np.float32(float(self.in_chans // self.num_heads) ** -0.5))
        # the host tables, fp64: the torch backend reads them; building them validates the grids
        hw, logw = A.attention_s2_tables(self.in_shape, self.out_shape, grid_in, grid_out, self.theta_cutoff,
                                         dtype=np.float64)
        self._hw, self._logw64 = torch.from_numpy(hw), torch.from_numpy(logw)
        C, s = self.in_chans, 1.0 / math.sqrt(self.in_chans)
        self.q_weight = nn.Parameter(s * torch.randn(C, C))
        self.k_weight = nn.Parameter(s * torch.randn(C, C))
        self.v_weight = nn.Parameter(s * torch.randn(C, C))
        self.proj_weight = nn.Parameter(s * torch.randn(self.out_chans, C))
        for n, c in (("q", C), ("k", C), ("v", C), ("proj", self.out_chans)):
            setattr(self, n + "_bias", nn.Parameter(torch.zeros(c)) if bias else None)

    def set_backend(self, backend: str) -> "NeighborhoodAttentionS2":
        if backend not in ("torch", "amd"):
            raise ValueError(f"backend must be 'torch' or 'amd', got {backend!r}")
        self.backend = backend
        return self

    def extra_repr(self) -> str:
        return (f"{self.in_chans}, in_shape={self.in_shape}, out_shape={self.out_shape}, num_heads={self.num_heads}, "
                f"grid_in={self.grid_in!r}, grid_out={self.grid_out!r}, theta_cutoff={self.theta_cutoff:.6g}, "
                f"out_chans={self.out_chans}, backend={self.backend!r}")

    def tables(self, device) -> "A._AttentionS2Tables":
        return A.attention_s2_table_holder(self.in_shape, self.out_shape, self.grid_in, self.grid_out,
                                           self.theta_cutoff, device)

    # ---- torch backend: the definition
    def attend_torch(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """The attention step alone in q's precision: a masked softmax over the band of input rows of one output
        latitude at a time."""
        B, H = q.shape[0], self.num_heads
        (Hi, Wi), (Ho, Wo) = self.in_shape, self.out_shape
        d, s = self.in_chans // H, Wi // Wo
        qh, kh, vh = q.reshape(B, H, d, Ho, Wo), k.reshape(B, H, d, Hi, Wi), v.reshape(B, H, d, Hi, Wi)
        logw = self._logw64.to(device=q.device, dtype=q.dtype)
        off = (torch.arange(Wi)[None, :] - s * torch.arange(Wo)[:, None]) % Wi
        circ = torch.minimum(off, Wi - off)  # [Wo, Wi]
        y = q.new_zeros(B, H, d, Ho, Wo)
        for ko in range(Ho):
            rows = torch.nonzero(self._hw[ko] >= 0).flatten()
            if len(rows) == 0:
                continue
            mask = (circ[:, None, :] <= self._hw[ko, rows].long()[None, :, None]).to(q.device)  # [Wo, rows, Wi]
            score = self.scale * torch.einsum("bhcq,bhckj->bhqkj", qh[:, :, :, ko], kh[:, :, :, rows])
            score = (score + logw[rows][:, None]).masked_fill(~mask, float("-inf"))
            p = torch.softmax(score.flatten(3), dim=-1).reshape(score.shape)
            y[:, :, :, ko] = torch.einsum("bhqkj,bhckj->bhcq", p, vh[:, :, :, rows])
        return y.reshape(B, H * d, Ho, Wo)

    def _forward_torch(self, query, key, value):
        if query.dtype == torch.bfloat16:
            return self._forward_torch(query.float(), key.float(), value.float()).to(torch.bfloat16)
        dt = query.dtype

        def lin(x, w, b):
            y = torch.einsum("oc,bckj->bokj", w.to(dt), x)
            return y if b is None else y + b.to(dt)[None, :, None, None]

        y = self.attend_torch(lin(query, self.q_weight, self.q_bias), lin(key, self.k_weight, self.k_bias),
                              lin(value, self.v_weight, self.v_bias))
        return lin(y, self.proj_weight, self.proj_bias)

    # ---- amd backend
    def _f32(self, name: str):
        from ..ops.spectral import module_cached

        p = getattr(self, name)
        return None if p is None else module_cached(self, name + "_f32", (p,),
                                                    lambda: p.detach().float().contiguous())

    def _forward_amd(self, query, key, value):
        if query.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"NeighborhoodAttentionS2: the amd backend takes float32 or bfloat16, got {query.dtype}")
        if not (query.dtype == key.dtype == value.dtype):
            raise TypeError("NeighborhoodAttentionS2: query, key and value must share one dtype")
        pw = torch.ops.amd_dft.fno_pointwise
        q = pw(None, query, self._f32("q_weight"), self._f32("q_bias"), False)
        k = pw(None, key, self._f32("k_weight"), self._f32("k_bias"), False)
        v = pw(None, value, self._f32("v_weight"), self._f32("v_bias"), False)
        y = A.attention_s2(q, k, v, self.tables(query.device), self.scale, self.num_heads)
        return pw(None, y, self._f32("proj_weight"), self._f32("proj_bias"), False)

    def forward(self, query: torch.Tensor, key: Optional[torch.Tensor] = None,
                value: Optional[torch.Tensor] = None) -> torch.Tensor:
        if key is None:
            if self.in_shape != self.out_shape:
                raise ValueError("NeighborhoodAttentionS2: self-attention needs equal grids; pass key (and value)")
            key = query
        if value is None:
            value = key
        want_q, want_k = (self.in_chans,) + self.out_shape, (self.in_chans,) + self.in_shape
        if query.dim() != 4 or tuple(query.shape[1:]) != want_q or key.dim() != 4 or \
                tuple(key.shape[1:]) != want_k or value.shape != key.shape or key.shape[0] != query.shape[0]:
            raise ValueError(f"NeighborhoodAttentionS2: expected query [B, {want_q}] and key, value [B, {want_k}], "
                             f"got {tuple(query.shape)}, {tuple(key.shape)} and {tuple(value.shape)}")
        fwd = self._forward_amd if self.backend == "amd" else self._forward_torch
        return fwd(query, key, value)


class AttentionS2(nn.Module):
    """Global attention on the sphere.  ``forward(query, key=None, value=None)``: ``query`` [B, in_chans, nlat_out,
    nlon_out], ``key`` and ``value`` [B, in_chans, nlat_in, nlon_in] (``key`` defaults to ``query`` where the grids are
    equal, ``value`` to ``key``) -> [B, out_chans, nlat_out, nlon_out].  The grids need no relation to each other."""

    def __init__(self, in_chans: int, in_shape: Tuple[int, int], out_shape: Tuple[int, int], num_heads: int = 1,
                 grid_in: str = "equiangular", grid_out: str = "equiangular", bias: bool = True,
                 out_chans: Optional[int] = None, backend: str = "amd"):
        super().__init__()
        self.in_chans = int(in_chans)
        self.out_chans = int(out_chans) if out_chans is not None else self.in_chans
        self.num_heads = int(num_heads)
        if self.num_heads < 1 or self.in_chans % self.num_heads:
            raise ValueError(f"in_chans ({self.in_chans}) must be a multiple of num_heads ({self.num_heads})")
        self.in_shape = tuple(int(v) for v in in_shape)
        self.out_shape = tuple(int(v) for v in out_shape)
        if grid_out not in A.GRIDS or min(self.out_shape) < 1:
            raise ValueError(f"grid_out must be one of {A.GRIDS} and out_shape positive, got {grid_out!r}, "
                             f"{self.out_shape}")
        self.grid_in, self.grid_out = grid_in, grid_out
        self.set_backend(backend)
        # d ** -0.5 as fp32: the value the kernel takes and an exported graph's float attribute carries
        self.scale = float(np.float32(float(self.in_chans // self.num_heads) ** -0.5))
        # fp64, for the torch backend; building it validates the input grid
        self._logw64 = torch.from_numpy(A.attention_s2_global_tables(self.in_shape, grid_in, dtype=np.float64))
        C, s = self.in_chans, 1.0 / math.sqrt(self.in_chans)
        self.q_weight = nn.Parameter(s * torch.randn(C, C))
        self.k_weight = nn.Parameter(s * torch.randn(C, C))
        self.v_weight = nn.Parameter(s * torch.randn(C, C))
        self.proj_weight = nn.Parameter(s * torch.randn(self.out_chans, C))
        for n, c in (("q", C), ("k", C), ("v", C), ("proj", self.out_chans)):
            setattr(self, n + "_bias", nn.Parameter(torch.zeros(c)) if bias else None)

    def set_backend(self, backend: str) -> "AttentionS2":
        if backend not in ("torch", "amd"):
            raise ValueError(f"backend must be 'torch' or 'amd', got {backend!r}")
        self.backend = backend
        return self

    def extra_repr(self) -> str:
        return (f"{self.in_chans}, in_shape={self.in_shape}, out_shape={self.out_shape}, num_heads={self.num_heads}, "
                f"grid_in={self.grid_in!r}, grid_out={self.grid_out!r}, out_chans={self.out_chans}, "
                f"backend={self.backend!r}")

    def tables(self, device) -> "A._AttentionS2GlobalTables":
        return A.attention_s2_global_table_holder(self.in_shape, self.grid_in, device)

    # ---- torch backend: the definition
    def attend_torch(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """The attention step alone in q's precision: one softmax over all input points."""
        B, H = q.shape[0], self.num_heads
        d = self.in_chans // H
        qh, kh, vh = q.reshape(B, H, d, -1), k.reshape(B, H, d, -1), v.reshape(B, H, d, -1)
        logw = self._logw64.to(device=q.device, dtype=q.dtype).repeat_interleave(self.in_shape[1])
        p = torch.softmax(self.scale * torch.einsum("bhcq,bhck->bhqk", qh, kh) + logw, dim=-1)
        return torch.einsum("bhqk,bhck->bhcq", p, vh).reshape(q.shape)

    _forward_torch = NeighborhoodAttentionS2._forward_torch
    _f32 = NeighborhoodAttentionS2._f32

    def _forward_amd(self, query, key, value):
        if query.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"AttentionS2: the amd backend takes float32 or bfloat16, got {query.dtype}")
        if not (query.dtype == key.dtype == value.dtype):
            raise TypeError("AttentionS2: query, key and value must share one dtype")
        pw = torch.ops.amd_dft.fno_pointwise
        q = pw(None, query, self._f32("q_weight"), self._f32("q_bias"), False)
        k = pw(None, key, self._f32("k_weight"), self._f32("k_bias"), False)
        v = pw(None, value, self._f32("v_weight"), self._f32("v_bias"), False)
        y = A.attention_s2_global(q, k, v, self.tables(query.device), self.scale, self.num_heads)
        return pw(None, y, self._f32("proj_weight"), self._f32("proj_bias"), False)

    def forward(self, query: torch.Tensor, key: Optional[torch.Tensor] = None,
                value: Optional[torch.Tensor] = None) -> torch.Tensor:
        if key is None:
            if self.in_shape != self.out_shape:
                raise ValueError("AttentionS2: self-attention needs equal grids; pass key (and value)")
            key = query
        if value is None:
            value = key
        want_q, want_k = (self.in_chans,) + self.out_shape, (self.in_chans,) + self.in_shape
        if query.dim() != 4 or tuple(query.shape[1:]) != want_q or key.dim() != 4 or \
                tuple(key.shape[1:]) != want_k or value.shape != key.shape or key.shape[0] != query.shape[0]:
            raise ValueError(f"AttentionS2: expected query [B, {want_q}] and key, value [B, {want_k}], "
                             f"got {tuple(query.shape)}, {tuple(key.shape)} and {tuple(value.shape)}")
        fwd = self._forward_amd if self.backend == "amd" else self._forward_torch
        return fwd(query, key, value)
