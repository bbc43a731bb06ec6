"""LayerNorm over the channels of channel-first fields, and the pre-norm MLP of a transformer block on them.

``ChannelLayerNorm``: ``y[b, c, ...] = (x[b, c, ...] - mean[b, ...]) * rsqrt(var[b, ...] + eps) * weight[c] + bias[c]``
with the mean and the biased variance over ``c`` -- ``nn.LayerNorm(C)`` applied to the channel dimension of a
``[B, C, *spatial]`` tensor without the two permutes.

``PreNormMLP``: ``h + fc2(GELU(fc1(LN(h))))`` with 1x1 convolutions ``fc1: embed -> hidden`` and
``fc2: hidden -> embed``.

Backends: ``"amd"`` (the default): ``ChannelLayerNorm`` is the ``layer_norm_nchw`` op
(``csrc/spectral/layer_norm_nchw.hip`` on a GPU, fp64 ATen math on CPU tensors); ``PreNormMLP`` is exactly two
kernels, ``fno_pointwise_ln`` (the LayerNorm applied as the MFMA 1x1 convolution stages its input: the normalised
tensor is never stored; GELU on) and ``fno_pointwise`` with ``spec = h``.  fp32 or bf16, no ATen fallback, so both run
under ``strict_mode``.  ``"torch"``: the definition in plain torch, in the input's precision (fp64 included).  Both
export through the generic ``com.amd.dft`` symbolic and run in ``OnnxGraph``.  No autograd on the amd backend."""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = ["ChannelLayerNorm", "PreNormMLP"]


def _check_backend(backend: str) -> str:
    if backend not in ("torch", "amd"):
        raise ValueError(f"backend must be 'torch' or 'amd', got {backend!r}")
    return backend


def _ln_torch(x: torch.Tensor, weight, bias, eps: float) -> torch.Tensor:
    if x.dtype == torch.bfloat16:
        return _ln_torch(x.float(), weight, bias, eps).to(torch.bfloat16)
    y = F.layer_norm(x.movedim(1, -1), (x.shape[1],), None if weight is None else weight.to(x.dtype),
                     None if bias is None else bias.to(x.dtype), eps)
    return y.movedim(-1, 1).contiguous()


def _f32(owner: nn.Module, name: str):
    from ..ops.spectral import module_cached

    p = getattr(owner, name)
    return None if p is None else module_cached(owner, name + "_f32", (p,), lambda: p.detach().float().contiguous())


def _amd_dtype(who: str, x: torch.Tensor) -> None:
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{who}: the amd backend takes float32 or bfloat16, got {x.dtype}")


class ChannelLayerNorm(nn.Module):
    """LayerNorm over dimension 1 of ``[B, num_channels, *spatial]``."""

    def __init__(self, num_channels: int, eps: float = 1e-5, affine: bool = True, backend: str = "amd"):
        super().__init__()
        self.num_channels, self.eps = int(num_channels), float(eps)
        if self.num_channels < 1:
            raise ValueError(f"num_channels must be >= 1, got {num_channels}")
        self.backend = _check_backend(backend)
        self.weight = nn.Parameter(torch.ones(self.num_channels)) if affine else None
        self.bias = nn.Parameter(torch.zeros(self.num_channels)) if affine else None

    def set_backend(self, backend: str) -> "ChannelLayerNorm":
        self.backend = _check_backend(backend)
        return self

    def extra_repr(self) -> str:
        return f"{self.num_channels}, eps={self.eps}, affine={self.weight is not None}, backend={self.backend!r}"

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() < 2 or x.shape[1] != self.num_channels:
            raise ValueError(f"ChannelLayerNorm: expected [B, {self.num_channels}, ...], got {tuple(x.shape)}")
        if self.backend == "torch":
            return _ln_torch(x, self.weight, self.bias, self.eps)
        _amd_dtype("ChannelLayerNorm", x)
        from ..ops import spectral as SP  # looked up per call, as SFNONet's norms are

        return SP.layer_norm_nchw(x, _f32(self, "weight"), _f32(self, "bias"), self.eps)


class PreNormMLP(nn.Module):
    """``h + fc2(GELU(fc1(LN(h))))`` on ``[B, embed, *spatial]``: LayerNorm over the channels, two 1x1 convolutions
    with biases, erf-GELU between them, the residual added in the second kernel."""

    def __init__(self, embed: int, hidden: int, eps: float = 1e-5, backend: str = "amd"):
        super().__init__()
        self.embed, self.hidden, self.eps = int(embed), int(hidden), float(eps)
        if self.embed < 1 or self.hidden < 1:
            raise ValueError(f"embed and hidden must be >= 1, got {embed}, {hidden}")
        self.backend = _check_backend(backend)
        self.norm_weight = nn.Parameter(torch.ones(self.embed))
        self.norm_bias = nn.Parameter(torch.zeros(self.embed))
        self.fc1_weight = nn.Parameter(torch.randn(self.hidden, self.embed) / math.sqrt(self.embed))
        self.fc1_bias = nn.Parameter(torch.zeros(self.hidden))
        self.fc2_weight = nn.Parameter(torch.randn(self.embed, self.hidden) / math.sqrt(self.hidden))
        self.fc2_bias = nn.Parameter(torch.zeros(self.embed))

    def set_backend(self, backend: str) -> "PreNormMLP":
        self.backend = _check_backend(backend)
        return self

    def extra_repr(self) -> str:
        return f"{self.embed}, {self.hidden}, eps={self.eps}, backend={self.backend!r}"

    def _forward_torch(self, h: torch.Tensor) -> torch.Tensor:
        if h.dtype == torch.bfloat16:
            return self._forward_torch(h.float()).to(torch.bfloat16)
        dt = h.dtype

        def lin(x, w, b):
            return torch.einsum("oc,bc...->bo...", w.to(dt), x) + b.to(dt).reshape(1, -1, *([1] * (x.dim() - 2)))

        t = F.gelu(lin(_ln_torch(h, self.norm_weight, self.norm_bias, self.eps), self.fc1_weight, self.fc1_bias))
        return h + lin(t, self.fc2_weight, self.fc2_bias)

    def _forward_amd(self, h: torch.Tensor) -> torch.Tensor:
        _amd_dtype("PreNormMLP", h)
        from ..ops import spectral as SP

        t = SP.fno_pointwise_ln(None, h, _f32(self, "norm_weight"), _f32(self, "norm_bias"), self.eps,
                                _f32(self, "fc1_weight"), _f32(self, "fc1_bias"), True)
        return torch.ops.amd_dft.fno_pointwise(h, t, _f32(self, "fc2_weight"), _f32(self, "fc2_bias"), False)

    def forward(self, h: torch.Tensor) -> torch.Tensor:
        if h.dim() < 2 or h.shape[1] != self.embed:
            raise ValueError(f"PreNormMLP: expected [B, {self.embed}, ...], got {tuple(h.shape)}")
        return self._forward_amd(h) if self.backend == "amd" else self._forward_torch(h)
