"""Host-side packer of the tinychat W4 x16 y16 weight format (role of the reference's
``nunchaku/models/text_encoders/tinychat_utils.py``; same names and signatures, written for this package).

Format, per linear layer of ``N`` outputs and ``K`` inputs quantised in groups of ``group_size``:

- ``qweight`` int16 ``[N/4, K]``: output channels in row groups of four.  A row group holds, for every 64-input chunk, the
  16 int16 of its row 0, then rows 1, 2, 3; of a row's 16 int16, number ``8h + j`` (h = 0, 1; j = 0..7) carries the
  4-bit codes of inputs ``32h + j, 32h + 8 + j, 32h + 16 + j, 32h + 24 + j`` of the chunk in nibbles 0..3.
- ``scales`` / ``scaled_zeros`` ``[ceil_num_groups, N]`` in the model dtype, rows past ``K / group_size`` zero;
  ``w = q * scale + scaled_zero`` (the zero point enters scaled and negated).
"""

import torch

__all__ = ["ceil_num_groups", "convert_to_tinychat_w4x16y16_linear_weight"]


def ceil_num_groups(in_features: int, group_size: int, weight_bits: int = 4) -> int:
    """Number of scale rows the tinychat kernels expect: ``in_features / group_size`` rounded up to whole int32 packs of
    codes (8 groups for 4 bits), and for groups of 64 / 32 to an even / fourfold number of packs."""
    if in_features % group_size:
        raise ValueError(f"in_features={in_features} is not a multiple of group_size={group_size}")
    if weight_bits not in (1, 2, 4):
        raise ValueError(f"weight_bits={weight_bits} (1, 2 or 4)")
    per_pack = 32 // weight_bits
    if group_size >= 128:
        factor = 1
    elif group_size in (64, 32):
        factor = 128 // group_size
    else:
        raise NotImplementedError(f"group_size={group_size} is not supported by the tinychat format")
    packs = -(-(in_features // group_size) // per_pack)
    packs = -(-packs // factor) * factor
    return packs * per_pack


def _pack_codes(codes: torch.Tensor) -> torch.Tensor:
    """``[N, K]`` integer codes in [0, 15] -> ``[N/4, K]`` int16 in the order of the module docstring."""
    n, k = codes.shape
    if n % 4 or k % 64:
        raise ValueError(f"codes [{n}, {k}]: need N % 4 == 0 and K % 64 == 0")
    c = codes.to(torch.int32).reshape(n, k // 32, 4, 8)  # [n][32-block][nibble e][j]: input 8e + j of the block
    words = c[:, :, 0] | (c[:, :, 1] << 4) | (c[:, :, 2] << 8) | (c[:, :, 3] << 12)  # [n][block][j]
    words = words.reshape(n // 4, 4, k // 64, 16).transpose(1, 2).reshape(n // 4, k)
    return words.to(torch.int16)  # (two's complement wrap of codes >= 8 in nibble 3)


def convert_to_tinychat_w4x16y16_linear_weight(weight: torch.Tensor, scale: torch.Tensor, zero: torch.Tensor, group_size: int = -1,
                                               zero_pre_scaled: bool = False) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Quantise ``weight`` [N, K] (fp16 / bf16, already on the quantisation grid) with per-group ``scale`` / ``zero``
    (``[N, K / group_size]`` or broadcastable scalars; ``zero`` in code units times ``scale`` unless ``zero_pre_scaled``,
    where it is in code units) and pack it: returns ``(qweight int16 [N/4, K], scales [G_pad, N], scaled_zeros [G_pad, N])``."""
    dtype, device = weight.dtype, weight.device
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"weight dtype {dtype}: the tinychat format holds fp16 / bf16 layers")
    if scale is None or zero is None:
        raise ValueError("scale and zero are both required")
    n, k = weight.shape
    gs = k if group_size <= 0 else group_size
    if gs > k or k % gs:
        raise ValueError(f"group_size={gs} does not divide in_features={k}")
    ng = k // gs
    s = scale.to(dtype=torch.float32, device=device)
    z = zero.to(dtype=torch.float32, device=device)
    if zero_pre_scaled:
        z = z * s
    s = (s.reshape(1, 1).expand(n, ng) if s.numel() == 1 else s.reshape(n, ng)).reshape(n, ng, 1)
    z = (z.reshape(1, 1).expand(n, ng) if z.numel() == 1 else z.reshape(n, ng)).reshape(n, ng, 1)
    q = torch.round((weight.to(torch.float32).reshape(n, ng, gs) + z) / s).reshape(n, k)
    if q.numel() and (q.min() < 0 or q.max() > 15):
        raise ValueError("weight is not on the 4-bit grid of scale / zero (codes outside [0, 15])")
    g_pad = ceil_num_groups(k, gs, weight_bits=4)
    scales = torch.zeros(g_pad, n, dtype=dtype, device=device)
    zeros = torch.zeros(g_pad, n, dtype=dtype, device=device)
    scales[:ng] = s.reshape(n, ng).t().to(dtype)
    zeros[:ng] = -z.reshape(n, ng).t().to(dtype)
    return _pack_codes(q.to(torch.int32)), scales, zeros
