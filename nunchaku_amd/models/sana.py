"""SANA's linear-attention layer (reference: src/SanaModel.cpp:13-136 ``SanaLinearAttention``).

The first part of the SANA family: the QKV projection, ReLU linear attention over its packed output (``svdq_linear_attention``: a new
kernel, where the reference folds the K/V reduction into the GEMM's epilogue with atomics) and the output projection.  The GLU-MBConv
with its depthwise convolution, the cross-attention, the block and the model class are not here yet.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from ..ops.attention import linear_attention
from .linear import SVDQW4A4Linear

HEAD_DIM = 32


class SanaLinearAttention(nn.Module):
    """``out_proj(linear_attention(qkv_proj(x)))`` with 32-channel heads.

    Sub-modules carry the reference's names (SanaModel.cpp:17-22): ``qkv_proj`` [dim_pad -> 3 * dim_pad], ``out_proj`` [dim_pad -> dim_pad] and,
    with ``pag``, ``pag_to_v`` [dim_pad -> dim_pad], where ``dim_pad = ceil(dim / 128) * 128``: the reference's 4-bit GEMM pads both feature
    counts to 128 (src/Linear.cpp:92-107), so a checkpoint's tensors already have the padded shapes (SANA-1.6B: 2240 -> 2304, 72 heads).
    Legacy key names are mapped by :func:`convert_sana_attention_state_dict`; the result loads with ``strict=True``.

    Tokens are NOT padded per batch element: the kernel takes ``T``.  The reference pads every batch element to 256 tokens with zero rows
    and sums over them, so with ``bias=True`` those rows would add ``relu(bias_k)`` and ``bias_v * relu(bias_k)`` to its ``vk``; here they do
    not exist.  SANA's attention has ``bias=False``, where the two agree."""

    def __init__(self, dim: int, bias: bool = False, pag: bool = False, rank: int = 32, torch_dtype: torch.dtype = torch.bfloat16,
                 device: str | torch.device | None = None):
        super().__init__()
        self.dim = dim
        self.dim_pad = (dim + 127) // 128 * 128
        self.heads = self.dim_pad // HEAD_DIM
        kw = dict(rank=rank, bias=bias, torch_dtype=torch_dtype, device=device)
        self.qkv_proj = SVDQW4A4Linear(self.dim_pad, 3 * self.dim_pad, **kw)
        self.out_proj = SVDQW4A4Linear(self.dim_pad, self.dim_pad, **kw)
        self.pag_to_v = SVDQW4A4Linear(self.dim_pad, self.dim_pad, **kw) if pag else None

    def _padded(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 3 or x.shape[-1] != self.dim:
            raise ValueError(f"SanaLinearAttention: expected x [B, T, {self.dim}], got {tuple(x.shape)}")
        return x if self.dim_pad == self.dim else F.pad(x, (0, self.dim_pad - self.dim))

    @staticmethod
    def _deliver(y: torch.Tensor, out: torch.Tensor | None) -> torch.Tensor:
        if out is None:
            return y
        out.copy_(y)
        return out

    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """x [B, T, dim] -> [B, T, dim] (into ``out`` when given)"""
        qkv = self.qkv_proj(self._padded(x))            # [B, T, 3 * dim_pad]: Q, then (K, V) per head
        attn = linear_attention(qkv, self.heads)        # [B, T, dim_pad], token-major
        return self._deliver(self.out_proj(attn)[..., : self.dim], out)

    def forward_pag(self, x: torch.Tensor, cfg: bool) -> torch.Tensor:
        """Perturbed-attention guidance (SanaModel.cpp:108-136): the first 2/3 (``cfg``) or the first half of the batch goes through
        :meth:`forward`, the rest -- the perturbed samples, whose attention is the identity -- through ``out_proj(pag_to_v(x))``."""
        if self.pag_to_v is None:
            raise RuntimeError("SanaLinearAttention.forward_pag: the layer was built without pag_to_v (pag=False)")
        B = x.shape[0]
        parts = 3 if cfg else 2
        if B % parts:
            raise ValueError(f"SanaLinearAttention.forward_pag: batch size {B} is not a multiple of {parts} (cfg={bool(cfg)})")
        n = B * (parts - 1) // parts
        out = torch.empty(B, x.shape[1], self.dim, dtype=x.dtype, device=x.device)
        self.forward(x[:n], out[:n])
        self._deliver(self.out_proj(self.pag_to_v(self._padded(x[n:])))[..., : self.dim], out[n:])
        return out


def convert_sana_attention_state_dict(sd: dict) -> dict:
    """Legacy parameter names -> this project's (what the reference's FLUX converter does, transformer_flux_v2.py:591-596, 623-628):
    ``lora_down`` -> ``proj_down``, ``lora_up`` -> ``proj_up``, ``smooth`` -> ``smooth_factor``, ``smooth_orig`` -> ``smooth_factor_orig``.
    Keys that already carry the new names pass through."""
    new = {}
    for k, v in sd.items():
        nk = k.replace(".lora_down", ".proj_down").replace(".lora_up", ".proj_up")
        if ".smooth_factor" not in k:
            if ".smooth_orig" in k:
                nk = nk.replace(".smooth_orig", ".smooth_factor_orig")
            elif ".smooth" in k:
                nk = nk.replace(".smooth", ".smooth_factor")
        new[nk] = v
    return new
