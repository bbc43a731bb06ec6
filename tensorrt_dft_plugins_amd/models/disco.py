"""``DiscreteContinuousConvS2``: the discrete-continuous (DISCO) convolution on the sphere, the local learned layer
of spherical U-Nets and local spherical neural operators, and the one that changes resolution (definition:
:mod:`..ops.disco`).

Backends: ``"amd"`` (the default): the ``disco`` op (``csrc/spectral/disco.hip`` on a GPU, its ATen counterpart on
CPU tensors) followed by one ``fno_pointwise`` over the ``Cin * K`` gathered channels.  ``"torch"``: the definition
and the numerics oracle, a sparse matrix applied at every output longitude in eager torch -- what a user writes
without the op; it follows the input's precision (fp64 in, fp64 out; a bf16 input is computed in fp32 and rounded
once).

The weight is ``[Cout, Cin, K]``, torch-harmonics' layout but not its normalisation: published weights do not
carry over.  ``DiscreteContinuousConvTransposeS2`` is the transposed (upsampling) layer, coarse grid -> fine grid:
one ``fno_pointwise`` at the coarse resolution, then the ``disco_t`` op (``csrc/spectral/disco_t.hip``), which adds
the bias.  Out of scope: ``groups``, other filter bases, autograd.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from ..ops import disco as D

__all__ = ["DiscreteContinuousConvS2", "DiscreteContinuousConvTransposeS2"]


class DiscreteContinuousConvS2(nn.Module):
    """``out[b, o, k', j'] = sum_{c, p} W[o, c, p] y[b, c, p, k', j'] + bias[o]`` with ``y = disco(x)``:
    [B, in_chans, nlat_in, nlon_in] -> [B, out_chans, nlat_out, nlon_out], fp32 or bf16 on the amd backend."""

    def __init__(self, in_chans: int, out_chans: int, in_shape: Tuple[int, int], out_shape: Tuple[int, int],
                 kernel_shape, bias: bool = True, grid_in: str = "equiangular", grid_out: str = "equiangular",
                 theta_cutoff: Optional[float] = None, normalize: bool = True, backend: str = "amd"):
        super().__init__()
        if backend not in ("torch", "amd"):
            raise ValueError(f"backend must be 'torch' or 'amd', got {backend!r}")
        self.in_chans, self.out_chans = int(in_chans), int(out_chans)
        self.in_shape = tuple(int(v) for v in in_shape)
        self.out_shape = tuple(int(v) for v in out_shape)
        self.kernel_shape = kernel_shape
        self.grid_in, self.grid_out = grid_in, grid_out
        self.theta_cutoff = (float(theta_cutoff) if theta_cutoff is not None
                             else D.default_cutoff(kernel_shape, self.out_shape[0]))
        self.normalize = bool(normalize)
        self.backend = backend
        self.K = D.kernel_size(kernel_shape)
        # the fp64 filter tensor, host: the torch backend casts it to the input's precision.  Building it also
        # validates the grids (ValueError for a bad grid or nlon_in % nlon_out != 0).
        rp, idx, val = D.disco_tables(self.in_shape, self.out_shape, kernel_shape, grid_in, grid_out,
                                      self.theta_cutoff, self.normalize, dtype=np.float64)
        rows = torch.repeat_interleave(torch.arange(len(rp) - 1), torch.from_numpy(np.diff(rp)).long())
        self._coo64 = (torch.stack([rows, torch.from_numpy(idx).long()]), torch.from_numpy(val))
        scale = 1.0 / math.sqrt(self.in_chans * self.K)
        self.weight = nn.Parameter(scale * torch.randn(self.out_chans, self.in_chans, self.K))
        self.bias = nn.Parameter(torch.zeros(self.out_chans)) if bias else None

    def set_backend(self, backend: str) -> "DiscreteContinuousConvS2":
        if backend not in ("torch", "amd"):
            raise ValueError(f"backend must be 'torch' or 'amd', got {backend!r}")
        self.backend = backend
        return self

    def extra_repr(self) -> str:
        return (f"{self.in_chans}, {self.out_chans}, in_shape={self.in_shape}, out_shape={self.out_shape}, "
                f"kernel_shape={self.kernel_shape}, grid_in={self.grid_in!r}, grid_out={self.grid_out!r}, "
                f"theta_cutoff={self.theta_cutoff:.6g}, normalize={self.normalize}, backend={self.backend!r}")

    def tables(self, device) -> "D._DiscoTables":
        return D.disco_table_holder(self.in_shape, self.out_shape, self.kernel_shape, self.grid_in, self.grid_out,
                                    self.theta_cutoff, self.normalize, device)

    # ---- torch backend: the definition
    def _psi(self, ref: torch.Tensor) -> torch.Tensor:
        cache = self.__dict__.setdefault("_psi_cache", {})
        key = (str(ref.device), ref.dtype)
        if key not in cache:
            ind, val = self._coo64
            size = (self.K * self.out_shape[0], self.in_shape[0] * self.in_shape[1])
            cache[key] = torch.sparse_coo_tensor(ind.to(ref.device), val.to(device=ref.device, dtype=ref.dtype),
                                                 size).coalesce()
        return cache[key]

    def gather_torch(self, x: torch.Tensor) -> torch.Tensor:
        """y [B, Cin, K, nlat_out, nlon_out] in x's precision: the sparse filter tensor applied to x rolled by
        s j' longitudes, one output longitude at a time."""
        B, C = x.shape[0], x.shape[1]
        (Hi, Wi), (Ho, Wo) = self.in_shape, self.out_shape
        s = Wi // Wo
        psi = self._psi(x)
        cols = []
        for j in range(Wo):
            xs = torch.roll(x, -s * j, dims=-1).reshape(B * C, Hi * Wi)
            cols.append(torch.sparse.mm(psi, xs.t()))  # [K Ho, B C]
        y = torch.stack(cols, dim=-1)  # [K Ho, B C, Wo]
        return y.reshape(self.K, Ho, B, C, Wo).permute(2, 3, 0, 1, 4)

    def _forward_torch(self, x: torch.Tensor) -> torch.Tensor:
        if x.dtype == torch.bfloat16:
            return self._forward_torch(x.float()).to(torch.bfloat16)
        y = self.gather_torch(x)
        out = torch.einsum("ocp,bcpkj->bokj", self.weight.to(x.dtype), y)
        if self.bias is not None:
            out = out + self.bias.to(x.dtype)[None, :, None, None]
        return out

    # ---- amd backend
    def _flat_weight(self):
        from ..ops.spectral import module_cached

        w = module_cached(self, "w_flat", (self.weight,),
                          lambda: self.weight.detach().float().reshape(self.out_chans, -1).contiguous())
        if self.bias is None:
            return w, None
        return w, module_cached(self, "b_f32", (self.bias,), lambda: self.bias.detach().float().contiguous())

    def _forward_amd(self, x: torch.Tensor) -> torch.Tensor:
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"DiscreteContinuousConvS2: the amd backend takes float32 or bfloat16, got {x.dtype}")
        B = x.shape[0]
        Ho, Wo = self.out_shape
        y = D.disco(x, self.tables(x.device))  # [B, Cin, K, Ho, Wo]
        w, b = self._flat_weight()
        return torch.ops.amd_dft.fno_pointwise(None, y.view(B, self.in_chans * self.K, Ho, Wo), w, b, False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4 or x.shape[1] != self.in_chans or tuple(x.shape[2:]) != self.in_shape:
            raise ValueError(f"DiscreteContinuousConvS2: expected [B, {self.in_chans}, {self.in_shape[0]}, "
                             f"{self.in_shape[1]}], got {tuple(x.shape)}")
        return self._forward_amd(x) if self.backend == "amd" else self._forward_torch(x)


class DiscreteContinuousConvTransposeS2(nn.Module):
    """The transposed (upsampling) layer: ``z[b, o, p, k', j'] = sum_c W[o, c, p] x[b, c, k', j']``, then
    ``out[b, o] = disco_t(z)[b, o] + bias[o]``: [B, in_chans, nlat_in, nlon_in] -> [B, out_chans, nlat_out,
    nlon_out] with ``nlon_out % nlon_in == 0``, fp32 or bf16 on the amd backend.

    Backends: ``"amd"``: one ``fno_pointwise`` at the coarse resolution (``Cin -> Cout * K``, no bias), then the
    ``disco_t`` op, which adds the bias (``csrc/spectral/disco_t.hip`` on a GPU).  ``"torch"``: the definition, a
    sparse matrix applied once per input longitude shift in eager torch, in the input's precision (fp64 in, fp64
    out; bf16 computed in fp32 and rounded once).  The weight is ``[Cout, Cin, K]``, torch-harmonics' layout
    (``DiscreteContinuousConvTransposeS2``) but not its normalisation: published weights do not carry over."""

    def __init__(self, in_chans: int, out_chans: int, in_shape: Tuple[int, int], out_shape: Tuple[int, int],
                 kernel_shape, bias: bool = True, grid_in: str = "equiangular", grid_out: str = "equiangular",
                 theta_cutoff: Optional[float] = None, normalize: bool = True, backend: str = "amd"):
        super().__init__()
        if backend not in ("torch", "amd"):
            raise ValueError(f"backend must be 'torch' or 'amd', got {backend!r}")
        self.in_chans, self.out_chans = int(in_chans), int(out_chans)
        self.in_shape = tuple(int(v) for v in in_shape)
        self.out_shape = tuple(int(v) for v in out_shape)
        self.kernel_shape = kernel_shape
        self.grid_in, self.grid_out = grid_in, grid_out
        self.theta_cutoff = (float(theta_cutoff) if theta_cutoff is not None
                             else D.default_cutoff(kernel_shape, self.in_shape[0]))
        self.normalize = bool(normalize)
        self.backend = backend
        self.K = D.kernel_size(kernel_shape)
        # the fp64 table, host: the torch backend casts it to the input's precision.  Building it also validates
        # the grids (ValueError for a bad grid or nlon_out % nlon_in != 0).
        rp, idx, val = D.disco_transpose_tables(self.in_shape, self.out_shape, kernel_shape, grid_in, grid_out,
                                                self.theta_cutoff, self.normalize, dtype=np.float64)
        rows = torch.repeat_interleave(torch.arange(len(rp) - 1), torch.from_numpy(np.diff(rp)).long())
        self._coo64 = (torch.stack([rows, torch.from_numpy(idx).long()]), torch.from_numpy(val))
        scale = 1.0 / math.sqrt(self.in_chans * self.K)
        self.weight = nn.Parameter(scale * torch.randn(self.out_chans, self.in_chans, self.K))
        self.bias = nn.Parameter(torch.zeros(self.out_chans)) if bias else None

    def set_backend(self, backend: str) -> "DiscreteContinuousConvTransposeS2":
        if backend not in ("torch", "amd"):
            raise ValueError(f"backend must be 'torch' or 'amd', got {backend!r}")
        self.backend = backend
        return self

    def extra_repr(self) -> str:
        return (f"{self.in_chans}, {self.out_chans}, in_shape={self.in_shape}, out_shape={self.out_shape}, "
                f"kernel_shape={self.kernel_shape}, grid_in={self.grid_in!r}, grid_out={self.grid_out!r}, "
                f"theta_cutoff={self.theta_cutoff:.6g}, normalize={self.normalize}, backend={self.backend!r}")

    def tables(self, device) -> "D._DiscoTransposeTables":
        return D.disco_transpose_table_holder(self.in_shape, self.out_shape, self.kernel_shape, self.grid_in,
                                              self.grid_out, self.theta_cutoff, self.normalize, device)

    # ---- torch backend: the definition
    def _psi(self, ref: torch.Tensor) -> torch.Tensor:
        cache = self.__dict__.setdefault("_psi_cache", {})
        key = (str(ref.device), ref.dtype)
        if key not in cache:
            ind, val = self._coo64
            s = self.out_shape[1] // self.in_shape[1]
            size = (self.out_shape[0] * s, self.K * self.in_shape[0] * self.in_shape[1])
            cache[key] = torch.sparse_coo_tensor(ind.to(ref.device), val.to(device=ref.device, dtype=ref.dtype),
                                                 size).coalesce()
        return cache[key]

    def gather_torch(self, z: torch.Tensor) -> torch.Tensor:
        """y [B, C, nlat_out, nlon_out] in z's precision from z [B, C, K, nlat_in, nlon_in]: the sparse table applied
        to z rolled by t input longitudes, which gives the output longitudes s t + rho, one t at a time."""
        B, C = z.shape[0], z.shape[1]
        (Hi, Wi), (Ho, Wo) = self.in_shape, self.out_shape
        s = Wo // Wi
        psi = self._psi(z)
        zk = z.permute(0, 1, 3, 2, 4)  # [B, C, Hi, K, Wi]: the table's k'-major column order
        cols = []
        for t in range(Wi):
            zs = torch.roll(zk, -t, dims=-1).reshape(B * C, Hi * self.K * Wi)
            cols.append(torch.sparse.mm(psi, zs.t()))  # [Ho s, B C]
        y = torch.stack(cols, dim=-1)  # [Ho s, B C, Wi]
        return y.reshape(Ho, s, B, C, Wi).permute(2, 3, 0, 4, 1).reshape(B, C, Ho, Wo)

    def _forward_torch(self, x: torch.Tensor) -> torch.Tensor:
        if x.dtype == torch.bfloat16:
            return self._forward_torch(x.float()).to(torch.bfloat16)
        z = torch.einsum("ocp,bckj->bopkj", self.weight.to(x.dtype), x)
        out = self.gather_torch(z)
        if self.bias is not None:
            out = out + self.bias.to(x.dtype)[None, :, None, None]
        return out

    # ---- amd backend
    def _flat_weight(self):
        from ..ops.spectral import module_cached

        w = module_cached(self, "w_flat", (self.weight,),
                          lambda: self.weight.detach().float().permute(0, 2, 1).reshape(self.out_chans * self.K, -1)
                          .contiguous())
        if self.bias is None:
            return w, None
        return w, module_cached(self, "b_f32", (self.bias,), lambda: self.bias.detach().float().contiguous())

    def _forward_amd(self, x: torch.Tensor) -> torch.Tensor:
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"DiscreteContinuousConvTransposeS2: the amd backend takes float32 or bfloat16, "
                            f"got {x.dtype}")
        B = x.shape[0]
        Hi, Wi = self.in_shape
        w, b = self._flat_weight()
        z = torch.ops.amd_dft.fno_pointwise(None, x, w, None, False)  # [B, Cout K, Hi, Wi]
        return D.disco_transpose(z.view(B, self.out_chans, self.K, Hi, Wi), self.tables(x.device), b)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4 or x.shape[1] != self.in_chans or tuple(x.shape[2:]) != self.in_shape:
            raise ValueError(f"DiscreteContinuousConvTransposeS2: expected [B, {self.in_chans}, {self.in_shape[0]}, "
                             f"{self.in_shape[1]}], got {tuple(x.shape)}")
        return self._forward_amd(x) if self.backend == "amd" else self._forward_torch(x)
