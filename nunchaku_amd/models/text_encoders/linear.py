"""W4Linear: AWQ 4-bit weight, 16-bit activation linear layer of the quantised T5 encoder (role of the reference's
``nunchaku/models/text_encoders/linear.py``: same constructor, buffer names, shapes and dtypes, so its checkpoints load
unchanged).  ``forward`` is one ``ops.gemm_awq`` launch for every number of rows, with the bias fused."""

import torch
import torch.nn as nn

from ..._C import ops
from .tinychat_utils import ceil_num_groups, convert_to_tinychat_w4x16y16_linear_weight

__all__ = ["W4Linear"]


class W4Linear(nn.Module):
    """Buffers: ``qweight`` int16 ``[out/4, in]`` (tinychat order), ``scales`` / ``scaled_zeros`` ``[ceil_num_groups, out]``,
    ``bias`` ``[out]`` or None.  ``weight`` is a plain attribute (not in the state dict), an empty tensor of the compute
    dtype: transformers' T5 feed-forward reads ``wo.weight.dtype`` to cast its input."""

    def __init__(self, in_features: int, out_features: int, bias: bool = False, group_size: int = 128,
                 dtype: torch.dtype = torch.float16, device: str | torch.device = "cuda"):
        super().__init__()
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"W4Linear: dtype {dtype} (float16 or bfloat16)")
        self.in_features, self.out_features = in_features, out_features
        self.group_size = in_features if group_size == -1 else group_size
        if in_features % self.group_size or out_features % self.interleave:
            raise ValueError(f"W4Linear: in_features={in_features} must be a multiple of group_size={self.group_size}, "
                             f"out_features={out_features} of {self.interleave}")
        self.ceil_num_groups = ceil_num_groups(in_features, self.group_size, self.weight_bits)
        self.register_buffer("qweight", torch.zeros(out_features // self.interleave, in_features // (16 // self.weight_bits) * self.interleave,
                                                    dtype=torch.int16, device=device))
        self.register_buffer("scales", torch.zeros(self.ceil_num_groups, out_features, dtype=dtype, device=device))
        self.register_buffer("scaled_zeros", torch.zeros(self.ceil_num_groups, out_features, dtype=dtype, device=device))
        if bias:
            self.register_buffer("bias", torch.zeros(out_features, dtype=dtype, device=device))
        else:
            self.bias = None
        self.weight = torch.empty(0, dtype=dtype, device="meta")

    @property
    def weight_bits(self) -> int:
        return 4

    @property
    def interleave(self) -> int:
        return 4

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.group_size != 128:
            raise NotImplementedError(f"W4Linear: group_size={self.group_size} (the AWQ GEMM kernel implements 128)")
        return ops.gemm_awq(x, self.qweight, self.scales, self.scaled_zeros, bias=self.bias)

    @staticmethod
    def from_linear(linear: nn.Linear, group_size: int, init_only: bool = False, weight: torch.Tensor | None = None,
                    scale: torch.Tensor | None = None, zero: torch.Tensor | None = None, zero_pre_scaled: bool = False) -> "W4Linear":
        """A W4Linear of ``linear``'s shape, dtype and device.  Unless ``init_only``: quantised from ``weight`` (default
        ``linear.weight``) with the given per-group ``scale`` / ``zero``, or -- neither given -- by asymmetric min / max
        quantisation per group of ``group_size`` inputs (codes 0..15)."""
        if not isinstance(linear, nn.Linear):
            raise TypeError("W4Linear.from_linear takes an nn.Linear")
        w = linear.weight.data if weight is None else weight.data
        dtype, device = w.dtype, w.device
        n, k = linear.out_features, linear.in_features
        q = W4Linear(k, n, bias=linear.bias is not None, group_size=group_size, dtype=dtype, device=device)
        if init_only:
            return q
        if linear.bias is not None:
            q.bias.copy_(linear.bias.data)
        if scale is None:
            if zero is not None:
                raise ValueError("W4Linear.from_linear: scale and zero come together")
            gs = k if group_size <= 0 else group_size
            if gs > k or k % gs:
                raise ValueError(f"group_size={gs} does not divide in_features={k}")
            wf = w.to(torch.float32).reshape(n, 1, k // gs, gs)
            lo, hi = wf.amin(dim=-1, keepdim=True), wf.amax(dim=-1, keepdim=True)
            scale = (hi - lo) / 15
            scale[scale == 0] = 1.0
            if zero_pre_scaled:
                zero = torch.clamp(torch.round(-lo / scale), 0, 15)
                wf = (torch.clamp(torch.round(wf / scale + zero), 0, 15) - zero) * scale
            else:
                zero = torch.clamp(-lo, min=0)
                wf = torch.clamp(torch.round((wf + zero) / scale), 0, 15) * scale - zero
            w = wf.to(dtype).reshape(n, k)
            scale, zero = scale.to(dtype), zero.to(dtype)
        qw, sc, zr = convert_to_tinychat_w4x16y16_linear_weight(w, scale, zero, group_size=group_size, zero_pre_scaled=zero_pre_scaled)
        q.qweight.copy_(qw)
        q.scales.copy_(sc)
        q.scaled_zeros.copy_(zr)
        return q

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"weight_bits={self.weight_bits}, group_size={self.group_size}")
