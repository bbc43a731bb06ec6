"""Spherical FNO (SFNO, Bonev et al. 2023; FourCastNet v2) layers on the MI355X spherical harmonic transform.

An SFNO layer is an FNO layer with the 2-D FFT replaced by a spherical harmonic transform (SHT): a real FFT along
longitude followed by a Legendre transform along latitude (conventions: :mod:`..ops.sht`).

* ``RealSHT`` / ``InverseRealSHT``: the torch-harmonics modules by name and argument order, complex tensors in and
  out, so they drop into code written against that package.
* ``RealVectorSHT`` / ``InverseRealVectorSHT``: the vector pair (tangential fields <-> spheroidal / toroidal
  coefficients; definitions and sign convention in :mod:`..ops.sht`), the same constructor arguments.
* ``SphericalConv2d``: the SFNO spectral operator, y[b,o,l,m] = sum_i x[b,i,l,m] w[i,o,l] (``operator="dhconv"``, one
  weight per degree: the Driscoll-Healy form) or sum_i x[b,i,l,m] w[i,o,l,m] (``operator="diagonal"``, one per mode).
* ``SFNOBlock``: ``act(SphericalConv2d(x) + Conv1x1(x))``.
* ``SFNONet`` / ``SFNOConfig``: a whole network of them (FourCastNet-v2 style): 1x1 encoder, position embedding,
  ``depth`` blocks of instance norm -> ``SFNOBlock`` -> instance norm -> 1x1 MLP with a residual, 1x1 decoder.

Backends: ``"amd"`` (the default: ``sht`` -> mix -> ``isht`` and the ``fno_pointwise`` tail, hand kernels on a
GPU, their ATen counterparts on CPU tensors) and ``"torch"`` (torch.fft + einsum on a table built in fp64: the
numerics oracle; it follows the input's precision, so an fp64 input gives an fp64 reference).

The mix of the amd backend is one of two ops (``mix=`` of the layers): ``fno_mix`` on the weights expanded over
every order m, or ``sfno_mix`` (csrc/spectral/sfno_mix.hip), which reads the per-degree weights directly -- one
bf16x3 MFMA GEMM per degree -- and needs no expansion.  ``"auto"`` expands up to ``EXPAND_LIMIT_BYTES`` and runs
``sfno_mix`` on device tensors above it; ``"degree"`` always runs ``sfno_mix``; ``"expand"`` always runs ``fno_mix``
on the expansion.  The per-mode operator (``operator="diagonal"``) is an ``fno_mix`` call as it stands.

Precision of the amd backend follows the input: fp32, or bf16 end to end (``sht``, the mix, ``isht`` and the
``fno_pointwise`` tail all take and return bf16; the bf16 mix is the per-degree kernel under ``"auto"`` and
``"degree"``, the bf16 ``fno_mix`` under ``"expand"`` and for the diagonal operator; the weights are cast, and
repacked or expanded, once per dtype and cached on the module).  ``RealSHT`` / ``InverseRealSHT`` have complex tensors at one end, and complex bf16 does not exist: they stay
fp32 / complex64, and bf16 callers use ``ops.sht.sht`` / ``isht`` (coefficients with a trailing re/im dim).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import sht as S

__all__ = ["RealSHT", "InverseRealSHT", "RealVectorSHT", "InverseRealVectorSHT", "SphericalConv2d", "SFNOBlock", "SFNOConfig", "SFNONet"]

# SphericalConv2d(mix="auto") expands its [Cin, Cout, lmax] weights over m for fno_mix; beyond this many bytes it
# does not, and mixes per degree; mix="expand" raises beyond it
EXPAND_LIMIT_BYTES = 256 << 20


def _check_mix(mix: str) -> str:
    if mix not in ("auto", "degree", "expand"):
        raise ValueError(f"mix must be 'auto', 'degree' or 'expand', got {mix!r}")
    return mix


def _check_operator(operator: str) -> str:
    if operator not in ("dhconv", "diagonal"):
        raise ValueError(f"operator must be 'dhconv' or 'diagonal', got {operator!r}")
    return operator


def _check_backend(backend: str) -> str:
    if backend not in ("torch", "amd"):
        raise ValueError(f"backend must be 'torch' or 'amd', got {backend!r}")
    return backend


class _SHTBase(nn.Module):
    def __init__(self, nlat: int, nlon: int, lmax: Optional[int] = None, mmax: Optional[int] = None,
                 grid: str = "equiangular", backend: str = "amd"):
        super().__init__()
        self.nlat, self.nlon, self.grid = int(nlat), int(nlon), grid
        self.lmax, self.mmax = S._defaults(self.nlat, self.nlon, lmax, mmax)
        self.backend = _check_backend(backend)
        _, w, P = S.legendre_tables(self.nlat, self.lmax, self.mmax, grid)
        self._table64 = self._make_table(w, P)  # fp64, host: the "torch" backend casts it to the input's precision

    def _table(self, ref: torch.Tensor) -> torch.Tensor:
        return self._table64.to(device=ref.device, dtype=ref.real.dtype if ref.is_complex() else ref.dtype)

    def extra_repr(self) -> str:
        return (f"nlat={self.nlat}, nlon={self.nlon}, lmax={self.lmax}, mmax={self.mmax}, grid={self.grid!r}, "
                f"backend={self.backend!r}")


class RealSHT(_SHTBase):
    """Forward real SHT: real [..., nlat, nlon] -> complex [..., lmax, mmax].  amd backend: fp32 only -- there is no
    complex bf16, so a bf16 field raises ``TypeError``; call ``sht`` (trailing re/im) instead."""

    @staticmethod
    def _make_table(w, P):
        return torch.from_numpy(P * w[None, None, :])  # [mmax, lmax, nlat]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.shape[-2] != self.nlat or x.shape[-1] != self.nlon:
            raise ValueError(f"RealSHT: expected a [..., {self.nlat}, {self.nlon}] grid, got {tuple(x.shape)}")
        if self.backend == "amd":
            if x.dtype == torch.bfloat16:
                raise TypeError("RealSHT: complex bfloat16 does not exist; for a bfloat16 field call sht() "
                                "(ops.sht.sht), which returns the coefficients with a trailing re/im dim")
            return torch.view_as_complex(S.sht(x, self.lmax, self.mmax, self.grid))
        xf = 2.0 * np.pi * torch.fft.rfft(x, dim=-1, norm="forward")[..., :self.mmax]
        c = torch.einsum("mlk,...kmc->...lmc", self._table(x), torch.view_as_real(xf))
        return torch.view_as_complex(c.contiguous())


class InverseRealSHT(_SHTBase):
    """Inverse real SHT: complex [..., lmax, mmax] -> real [..., nlat, nlon].  amd backend: complex64 only -- bf16
    coefficients (a real tensor with a trailing re/im dim) raise ``TypeError``; call ``isht`` instead."""

    @staticmethod
    def _make_table(w, P):
        return torch.from_numpy(np.ascontiguousarray(P.transpose(0, 2, 1)))  # [mmax, nlat, lmax]

    def forward(self, c: torch.Tensor) -> torch.Tensor:
        if self.backend == "amd" and c.dtype == torch.bfloat16:
            raise TypeError("InverseRealSHT: complex bfloat16 does not exist; for bfloat16 coefficients with a "
                            "trailing re/im dim call isht() (ops.sht.isht)")
        if c.shape[-2] != self.lmax or c.shape[-1] != self.mmax:
            raise ValueError(f"InverseRealSHT: expected [..., {self.lmax}, {self.mmax}] coefficients, got {tuple(c.shape)}")
        if self.backend == "amd":
            return S.isht(c, self.nlat, self.nlon, self.grid)
        xf = torch.einsum("mkl,...lmc->...kmc", self._table(c), torch.view_as_real(c))
        return torch.fft.irfft(torch.view_as_complex(xf.contiguous()), n=self.nlon, dim=-1, norm="forward")


class _VectorSHTBase(nn.Module):
    def __init__(self, nlat: int, nlon: int, lmax: Optional[int] = None, mmax: Optional[int] = None,
                 grid: str = "equiangular", backend: str = "amd"):
        super().__init__()
        self.nlat, self.nlon, self.grid = int(nlat), int(nlon), grid
        self.lmax, self.mmax = S._defaults(self.nlat, self.nlon, lmax, mmax)
        self.backend = _check_backend(backend)
        _, w, D0, D1 = S.vector_legendre_tables(self.nlat, self.lmax, self.mmax, grid)
        # fp64, host: the "torch" backend casts them to the input's precision
        self._a64, self._b64 = self._make_tables(w, D0, D1)

    def _transform(self, x: torch.Tensor) -> torch.Tensor:
        """The definition on a complex [..., 2, Q, M] tensor: y0 = A x0 - i B x1, y1 = A x1 + i B x0."""
        xr = torch.view_as_real(x)
        ta, tb = (t.to(device=x.device, dtype=xr.dtype) for t in (self._a64, self._b64))
        a = torch.view_as_complex(torch.einsum("mrq,...qmc->...rmc", ta, xr).contiguous())
        b = torch.view_as_complex(torch.einsum("mrq,...qmc->...rmc", tb, xr).contiguous())
        return torch.stack([a[..., 0, :, :] - 1j * b[..., 1, :, :], a[..., 1, :, :] + 1j * b[..., 0, :, :]], dim=-3)

    extra_repr = _SHTBase.extra_repr


class RealVectorSHT(_VectorSHTBase):
    """Forward vector SHT: real [..., 2, nlat, nlon] (v_theta, v_phi) -> complex [..., 2, lmax, mmax] (spheroidal,
    toroidal).  amd backend: fp32 only -- a bf16 field raises ``TypeError``; call ``vsht`` (trailing re/im) instead."""

    @staticmethod
    def _make_tables(w, D0, D1):
        l = np.arange(D0.shape[1], dtype=np.float64)
        norm = np.where(l > 0, 1.0 / np.maximum(1.0, l * (l + 1.0)), 0.0)[None, :, None] * w[None, None, :]
        return torch.from_numpy(D0 * norm), torch.from_numpy(D1 * norm)  # [mmax, lmax, nlat]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() < 3 or tuple(x.shape[-3:]) != (2, self.nlat, self.nlon):
            raise ValueError(f"RealVectorSHT: expected a [..., 2, {self.nlat}, {self.nlon}] field, got {tuple(x.shape)}")
        if self.backend == "amd":
            if x.dtype == torch.bfloat16:
                raise TypeError("RealVectorSHT: complex bfloat16 does not exist; for a bfloat16 field call vsht() "
                                "(ops.sht.vsht), which returns the coefficients with a trailing re/im dim")
            return torch.view_as_complex(S.vsht(x, self.lmax, self.mmax, self.grid))
        return self._transform(2.0 * np.pi * torch.fft.rfft(x, dim=-1, norm="forward")[..., :self.mmax])


class InverseRealVectorSHT(_VectorSHTBase):
    """Inverse vector SHT: complex [..., 2, lmax, mmax] -> real [..., 2, nlat, nlon].  amd backend: complex64 only --
    bf16 coefficients (a real tensor with a trailing re/im dim) raise ``TypeError``; call ``ivsht`` instead."""

    @staticmethod
    def _make_tables(w, D0, D1):
        return (torch.from_numpy(np.ascontiguousarray(D0.transpose(0, 2, 1))),
                torch.from_numpy(np.ascontiguousarray(D1.transpose(0, 2, 1))))  # [mmax, nlat, lmax]

    def forward(self, c: torch.Tensor) -> torch.Tensor:
        if self.backend == "amd" and c.dtype == torch.bfloat16:
            raise TypeError("InverseRealVectorSHT: complex bfloat16 does not exist; for bfloat16 coefficients with a "
                            "trailing re/im dim call ivsht() (ops.sht.ivsht)")
        if c.dim() < 3 or tuple(c.shape[-3:]) != (2, self.lmax, self.mmax):
            raise ValueError(f"InverseRealVectorSHT: expected [..., 2, {self.lmax}, {self.mmax}] coefficients, got "
                             f"{tuple(c.shape)}")
        if self.backend == "amd":
            return S.ivsht(c, self.nlat, self.nlon, self.grid)
        return torch.fft.irfft(self._transform(c), n=self.nlon, dim=-1, norm="forward")


class SphericalConv2d(nn.Module):
    """The SFNO spectral operator ``y = isht(mix(sht(x)))``.  ``operator`` picks the weights:

    * ``"dhconv"`` (the default, the Driscoll-Healy form): one complex weight per (in, out, degree l), shared by all
      orders m, ``mix[b,o,l,m] = sum_i c[b,i,l,m] w[i,o,l]``; ``weight`` is [Cin, Cout, lmax, 2].
    * ``"diagonal"``: one complex weight per (in, out, l, m), ``mix[b,o,l,m] = sum_i c[b,i,l,m] w[i,o,l,m]``;
      ``weight`` is [Cin, Cout, lmax, mmax, 2], initialised with the same scale.  The torch backend is
      ``einsum("bilm,iolm->bolm")`` in the input's precision; the amd backend runs ``sht`` -> ``fno_mix`` on the
      [.., lmax * mmax, 2] views -> ``isht``: fp32 on the fp32 weights, bf16 on the weights cast once and cached on
      the module (``w_diag_bf16``), bf16 end to end on the bf16 ``fno_mix`` kernels.  ``mix`` is ignored.

    The amd backend of ``"dhconv"`` runs ``sht`` -> mix -> ``isht``; ``mix`` picks the middle op:

    * ``"auto"`` (the default).  Up to 256 MiB of expanded weights (``EXPAND_LIMIT_BYTES``): ``fno_mix``, which
      takes one weight per mode, on the weights expanded over m once and cached on the module
      ([Cin, Cout, lmax * mmax, 2] fp32).  Above it the expansion is not built: a device tensor runs ``sfno_mix``
      (the per-degree MFMA kernel, ``tri=1`` since ``sht`` returns zeros where l < m) on the split weight table
      cached on the module (``w_degree``, as many bytes as the weights; rebuilt when the weights change, kept
      alive for captured graphs); a CPU tensor notes a ``sfno_mix`` fallback (not counted on CPU tensors) and mixes
      with ``torch.einsum``.
    * ``"degree"``: ``sfno_mix`` on every device and at every size; the expansion is never built.
    * ``"expand"``: ``fno_mix`` on the expansion, on every device and in both dtypes (a bf16 ``x`` mixes on the bf16
      ``fno_mix`` kernels with a bf16 expansion, ``w_expanded_bf16``, cached beside the fp32 one).  Above
      ``EXPAND_LIMIT_BYTES`` (counted in fp32 bytes for both dtypes) the forward raises ``ValueError``.

    A bf16 ``x`` runs bf16 end to end.  Under ``"auto"`` and ``"degree"`` that is ``sht`` -> ``sfno_mix`` -> ``isht``
    on every device and at every size: the bf16 ``"auto"`` never builds the expansion, although ``fno_mix`` has bf16
    kernels -- the per-degree kernel reads Cin * Cout * lmax weights where the expansion streams mmax times as many,
    and which of the two is faster depends on the shape (README, "bf16 fno_mix"), so the route that existing callers
    get stays the one they have.  Its tables (``w_bf16``, ``w_degree_bf16``: the weights rounded to bf16 once, and
    their one-plane repacked form) are cached beside the fp32 ones."""

    def __init__(self, in_ch: int, out_ch: int, nlat: int, nlon: int, lmax: Optional[int] = None,
                 mmax: Optional[int] = None, grid: str = "equiangular", backend: str = "amd", mix: str = "auto",
                 operator: str = "dhconv"):
        super().__init__()
        self.in_ch, self.out_ch = in_ch, out_ch
        self.mix = _check_mix(mix)
        self.operator = _check_operator(operator)
        self.sht = RealSHT(nlat, nlon, lmax, mmax, grid, backend)
        self.isht = InverseRealSHT(nlat, nlon, self.sht.lmax, self.sht.mmax, grid, backend)
        self.backend = _check_backend(backend)
        scale = 1.0 / (in_ch * out_ch)
        modes = (self.sht.lmax, self.sht.mmax) if self.operator == "diagonal" else (self.sht.lmax,)
        self.weight = nn.Parameter(scale * torch.rand(in_ch, out_ch, *modes, 2))

    def set_backend(self, backend: str) -> "SphericalConv2d":
        self.backend = self.sht.backend = self.isht.backend = _check_backend(backend)
        return self

    def expanded_bytes(self) -> int:
        return self.in_ch * self.out_ch * self.sht.lmax * self.sht.mmax * 2 * 4

    def _expanded_weight(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        from ..ops.spectral import module_cached

        L, M = self.sht.lmax, self.sht.mmax

        def build():
            w = self.weight.detach().to(dtype)
            return w[:, :, :, None, :].expand(-1, -1, -1, M, -1).reshape(self.in_ch, self.out_ch, L * M, 2).contiguous()

        return module_cached(self, "w_expanded" if dtype == torch.float32 else "w_expanded_bf16", (self.weight,), build)

    def _mode_weight(self, dtype: torch.dtype) -> torch.Tensor:
        """The diagonal operator's weights as ``fno_mix`` takes them, [Cin, Cout, lmax * mmax, 2]."""
        from ..ops.spectral import module_cached

        shape = (self.in_ch, self.out_ch, self.sht.lmax * self.sht.mmax, 2)
        if dtype == torch.float32:
            return self.weight.detach().float().reshape(shape)
        return module_cached(self, "w_diag_bf16", (self.weight,),
                             lambda: self.weight.detach().to(torch.bfloat16).reshape(shape).contiguous())

    def _degree_weight(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        from ..ops.spectral import module_cached, sfno_mix_split

        if dtype == torch.float32:
            return module_cached(self, "w_degree", (self.weight,), lambda: sfno_mix_split(self.weight))
        return module_cached(self, "w_degree_bf16", (self.weight,),
                             lambda: sfno_mix_split(self.weight.detach().to(torch.bfloat16)))

    def _weight_as(self, dtype: torch.dtype) -> torch.Tensor:
        from ..ops.spectral import module_cached

        if dtype == torch.float32:
            return self.weight.detach().float()
        return module_cached(self, "w_bf16", (self.weight,), lambda: self.weight.detach().to(torch.bfloat16))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.backend == "torch":
            wc = torch.view_as_complex(self.weight.to(x.dtype).contiguous())
            eq = "bilm,iolm->bolm" if self.operator == "diagonal" else "bilm,iol->bolm"
            return self.isht(torch.einsum(eq, self.sht(x), wc))
        from ..ops.spectral import fno_spectral_mix, note_fallback, sfno_mix

        B = x.shape[0]
        L, M = self.sht.lmax, self.sht.mmax
        c = S.sht(x, L, M, self.sht.grid)  # [B, Cin, L, M, 2], fp32 or bf16 as x
        dt = c.dtype
        if self.operator == "diagonal":
            y = fno_spectral_mix(c.reshape(B, self.in_ch, L * M, 2), self._mode_weight(dt))
            return S.isht(y.reshape(B, self.out_ch, L, M, 2), self.sht.nlat, self.sht.nlon, self.sht.grid)
        above = self.expanded_bytes() > EXPAND_LIMIT_BYTES
        if self.mix == "expand":
            if above:
                raise ValueError(f"SphericalConv2d(mix='expand'): the weights expanded over m take "
                                 f"{self.expanded_bytes()} bytes, above EXPAND_LIMIT_BYTES ({EXPAND_LIMIT_BYTES}); "
                                 "use mix='degree'")
            y = fno_spectral_mix(c.reshape(B, self.in_ch, L * M, 2), self._expanded_weight(dt))
            return S.isht(y.reshape(B, self.out_ch, L, M, 2), self.sht.nlat, self.sht.nlon, self.sht.grid)
        # bf16 under "auto": the per-degree kernel, as before fno_mix had bf16 kernels (class docstring)
        if self.mix == "degree" or dt == torch.bfloat16 or (above and x.is_cuda):
            y = sfno_mix(c, self._weight_as(dt), self._degree_weight(dt), tri=1)
        elif above:
            note_fallback("sfno_mix", "per-degree weights too large to expand over m for fno_mix: torch.einsum", x)
            wc = torch.view_as_complex(self.weight.float().contiguous())
            y = torch.view_as_real(torch.einsum("bilm,iol->bolm", torch.view_as_complex(c), wc)).contiguous()
        else:
            y = fno_spectral_mix(c.reshape(B, self.in_ch, L * M, 2), self._expanded_weight())
        return S.isht(y.reshape(B, self.out_ch, L, M, 2), self.sht.nlat, self.sht.nlon, self.sht.grid)


class SFNOBlock(nn.Module):
    """One SFNO layer: ``act(SphericalConv2d(x) + Conv1x1(x))``.  On the amd backend the tail (1x1 convolution,
    bias, the spectral addend and the GELU) is one ``fno_pointwise`` call.  ``mix`` and ``operator`` go to the
    ``SphericalConv2d`` (``"auto"``, ``"degree"`` or ``"expand"``; ``"dhconv"`` or ``"diagonal"``).  A bf16 ``x`` gives
    a bf16 layer: the bf16 ``SphericalConv2d`` and the bf16 ``fno_pointwise``."""

    def __init__(self, width: int, nlat: int, nlon: int, lmax: Optional[int] = None, mmax: Optional[int] = None,
                 grid: str = "equiangular", activation: bool = True, backend: str = "amd", mix: str = "auto",
                 operator: str = "dhconv"):
        super().__init__()
        self.spectral = SphericalConv2d(width, width, nlat, nlon, lmax, mmax, grid, backend, mix, operator)
        self.w = nn.Conv2d(width, width, 1)
        self.activation = activation
        self.backend = _check_backend(backend)

    def set_backend(self, backend: str) -> "SFNOBlock":
        self.backend = _check_backend(backend)
        self.spectral.set_backend(backend)
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        spec = self.spectral(x)
        if self.backend == "amd":
            return torch.ops.amd_dft.fno_pointwise(spec, x, self.w.weight.reshape(self.w.out_channels, -1).float(),
                                                   self.w.bias.float(), self.activation)
        y = spec.to(x.dtype) + self.w(x)
        return F.gelu(y) if self.activation else y


@dataclass
class SFNOConfig:
    img_size: Tuple[int, int] = (180, 360)  # (nlat, nlon)
    in_chans: int = 20
    out_chans: int = 20
    embed_dim: int = 64
    depth: int = 4
    lmax: Optional[int] = None
    mmax: Optional[int] = None
    grid: str = "equiangular"
    mlp_ratio: float = 2.0
    norm: str = "instance"  # "instance" | "none"
    pos_embed: bool = True
    mix: str = "auto"       # of the SphericalConv2d layers: "auto" | "degree" | "expand"
    eps: float = 1e-6
    operator: str = "dhconv"  # of the SphericalConv2d layers: "dhconv" | "diagonal"


def _conv1x1(conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """The 1x1 convolution in x's precision (the torch backend follows its input, fp64 included)."""
    return F.conv2d(x, conv.weight.to(x.dtype), conv.bias.to(x.dtype))


class SFNONetBlock(nn.Module):
    """One block of :class:`SFNONet`: ``h + fc2(GELU(fc1(IN1(SFNOBlock(IN0(h))))))``."""

    def __init__(self, cfg: SFNOConfig, lmax: int, mmax: int, backend: str):
        super().__init__()
        nlat, nlon = cfg.img_size
        E, hidden = cfg.embed_dim, int(round(cfg.mlp_ratio * cfg.embed_dim))
        instance = cfg.norm == "instance"
        self.norm0 = nn.InstanceNorm2d(E, eps=cfg.eps, affine=True) if instance else nn.Identity()
        self.layer = SFNOBlock(E, nlat, nlon, lmax, mmax, cfg.grid, True, backend, cfg.mix, cfg.operator)
        self.norm1 = nn.InstanceNorm2d(E, eps=cfg.eps, affine=True) if instance else nn.Identity()
        self.fc1 = nn.Conv2d(E, hidden, 1)
        self.fc2 = nn.Conv2d(hidden, E, 1)


class SFNONet(nn.Module):
    """A spherical FNO on an (nlat, nlon) grid, FourCastNet-v2 style, random init::

        h = enc2(GELU(enc1(x))) + pos              # 1x1 convs in_chans -> embed -> embed; pos [1, embed, nlat, nlon]
        for each block:
            n0 = IN0(h)
            a  = SFNOBlock(n0)                     # GELU(SphericalConv2d(n0) + Conv1x1(n0))
            n1 = IN1(a)
            h  = h + fc2(GELU(fc1(n1)))            # 1x1 convs embed -> mlp_ratio * embed -> embed
        y = dec2(GELU(dec1(h)))                    # embed -> embed -> out_chans

    GELU is the erf form; ``IN`` is ``nn.InstanceNorm2d(affine=True)`` (``norm="none"``: the identity); ``pos`` is
    left out with ``pos_embed=False``; ``mix`` and ``operator`` go to the ``SphericalConv2d`` layers.

    ``backend="torch"`` is the definition and the numerics oracle: it follows the input's precision, so an fp64 input
    gives an fp64 result.  ``backend="amd"`` (the default) runs every line on the hand kernels: each 1x1 convolution is
    one ``fno_pointwise`` call (its ``spec`` addend carries ``pos`` or the block's residual ``h``, its ``gelu`` flag the
    activation), the middle of a block is the :class:`SFNOBlock` path (``sht`` -> mix -> ``isht`` -> ``fno_pointwise``)
    and the norms are ``instance_norm`` (csrc/spectral/instance_norm.hip).  A bf16 input gives a bf16 network: bf16
    ``instance_norm``, the bf16 spherical line and the bf16 ``fno_pointwise``.  ``pos`` cast to the input's dtype and
    expanded over the batch is cached on the module per dtype and batch size.

    Out of scope: resolution changes between blocks (``scale_factor``), LayerNorm over NCHW, and weight-for-weight
    compatibility with any published checkpoint."""

    def __init__(self, cfg: Optional[SFNOConfig] = None, backend: str = "amd"):
        super().__init__()
        self.cfg = cfg = cfg or SFNOConfig()
        if cfg.norm not in ("instance", "none"):
            raise ValueError(f"norm must be 'instance' or 'none', got {cfg.norm!r}")
        _check_mix(cfg.mix)
        _check_operator(cfg.operator)
        nlat, nlon = (int(d) for d in cfg.img_size)
        lmax, mmax = S._defaults(nlat, nlon, cfg.lmax, cfg.mmax)
        E = cfg.embed_dim
        self.enc1 = nn.Conv2d(cfg.in_chans, E, 1)
        self.enc2 = nn.Conv2d(E, E, 1)
        self.pos = nn.Parameter(0.02 * torch.randn(1, E, nlat, nlon)) if cfg.pos_embed else None
        self.blocks = nn.ModuleList([SFNONetBlock(cfg, lmax, mmax, backend) for _ in range(cfg.depth)])
        self.dec1 = nn.Conv2d(E, E, 1)
        self.dec2 = nn.Conv2d(E, cfg.out_chans, 1)
        self.set_backend(backend)

    def set_backend(self, backend: str) -> "SFNONet":
        self.backend = _check_backend(backend)
        for b in self.blocks:
            b.layer.set_backend(backend)
        return self

    # ---- amd backend
    @staticmethod
    def _pw(conv: nn.Conv2d, x: torch.Tensor, gelu: bool, spec: Optional[torch.Tensor] = None) -> torch.Tensor:
        return torch.ops.amd_dft.fno_pointwise(spec, x, conv.weight.reshape(conv.out_channels, -1).float(),
                                               conv.bias.float(), gelu)

    def _pos_as(self, x: torch.Tensor) -> Optional[torch.Tensor]:
        from ..ops.spectral import module_cached

        if self.pos is None:
            return None
        B = int(x.shape[0])
        return module_cached(self, f"pos_{x.dtype}_{B}", (self.pos,),
                             lambda: self.pos.detach().to(x.dtype).expand(B, -1, -1, -1).contiguous())

    @staticmethod
    def _norm(n: nn.Module, x: torch.Tensor) -> torch.Tensor:
        if isinstance(n, nn.Identity):
            return x
        from ..ops import spectral as SP  # looked up per call, as the mix ops are (tests trace it)

        return SP.instance_norm(x, n.weight, n.bias, n.eps)

    def _forward_amd(self, x: torch.Tensor) -> torch.Tensor:
        from .._loader import load_plugins

        load_plugins()
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"SFNONet: the amd backend takes float32 or bfloat16, got {x.dtype}")
        h = self._pw(self.enc2, self._pw(self.enc1, x, True), False, self._pos_as(x))
        for b in self.blocks:
            a = b.layer(self._norm(b.norm0, h))
            h = self._pw(b.fc2, self._pw(b.fc1, self._norm(b.norm1, a), True), False, h)
        return self._pw(self.dec2, self._pw(self.dec1, h, True), False)

    # ---- torch backend: the definition
    @staticmethod
    def _norm_torch(n: nn.Module, x: torch.Tensor) -> torch.Tensor:
        if isinstance(n, nn.Identity):
            return x
        return F.instance_norm(x, weight=n.weight.to(x.dtype), bias=n.bias.to(x.dtype), eps=n.eps)

    def _forward_torch(self, x: torch.Tensor) -> torch.Tensor:
        h = _conv1x1(self.enc2, F.gelu(_conv1x1(self.enc1, x)))
        if self.pos is not None:
            h = h + self.pos.to(x.dtype)
        for b in self.blocks:
            n0 = self._norm_torch(b.norm0, h)
            a = F.gelu(b.layer.spectral(n0) + _conv1x1(b.layer.w, n0))
            n1 = self._norm_torch(b.norm1, a)
            h = h + _conv1x1(b.fc2, F.gelu(_conv1x1(b.fc1, n1)))
        return _conv1x1(self.dec2, F.gelu(_conv1x1(self.dec1, h)))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        nlat, nlon = self.cfg.img_size
        if x.dim() != 4 or x.shape[1] != self.cfg.in_chans or x.shape[2] != nlat or x.shape[3] != nlon:
            raise ValueError(f"SFNONet: expected [B, {self.cfg.in_chans}, {nlat}, {nlon}], got {tuple(x.shape)}")
        return self._forward_amd(x) if self.backend == "amd" else self._forward_torch(x)
