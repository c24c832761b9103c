"""OCP MXFP4 on the host: plain torch, CPU or GPU, not on the hot path (DESIGN.md section 6v states the format).

An element is e2m1 (4 bits ``s e e m``: +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}), two codes a byte with the even channel in the low nibble; a block of
32 consecutive channels shares one E8M0 scale byte ``2^(e - 127)``.  Of a block with largest magnitude ``amax`` (NaN ignored, +-inf counted as
the dtype's largest finite value) the byte is ``clamp(floor(log2 amax) - 2 + 127, 0, 254)`` (0 for an all-zero block) and a code is
``RNE_e2m1(v * 2^-(byte - 127))``: ties to the even mantissa, saturated to +-6, NaN -> 0, a value that rounds to zero is code 0 (no -0).
"""

from __future__ import annotations

import torch

E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
BLOCK = 32
# code c + 1 starts above (ties to c: even mantissa below) or at (ties to c + 1) the midpoint of the neighbours
_MIDPOINTS = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False))


def quantize_weight_mxfp4(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``w [rows, K]`` (16-bit or float; K a multiple of 32) -> ``(codes uint8 [rows, K/2], scales uint8 [K/32, rows])``, the checkpoint layout of
    ``SVDQW4A4Linear(precision="mxfp4")``'s ``qweight`` / ``wscales``.  Every step is exact in float64."""
    if w.dim() != 2 or w.shape[1] % BLOCK:
        raise ValueError("quantize_weight_mxfp4: expected [rows, K] with K a multiple of 32")
    top = torch.finfo(w.dtype).max if w.dtype.is_floating_point else float("inf")
    v = w.detach().double().reshape(w.shape[0], -1, BLOCK)
    mag = torch.nan_to_num(v.abs(), nan=0.0, posinf=top).clamp(max=top)
    amax = mag.amax(dim=-1)
    exp = torch.frexp(amax)[1] - 1  # floor(log2 amax) for amax > 0 (frexp: amax = m 2^e, 0.5 <= m < 1)
    byte = torch.where(amax > 0, (exp - 2 + 127).clamp(0, 254), torch.zeros_like(exp)).to(torch.int32)
    y = torch.ldexp(v, (127 - byte).unsqueeze(-1))  # v * 2^-(byte - 127); inf stays inf, NaN stays NaN
    ay = torch.nan_to_num(y.abs(), nan=0.0, posinf=6.0).clamp(max=6.0)
    code = torch.zeros_like(ay, dtype=torch.uint8)
    for mid, closed in _MIDPOINTS:
        code += (ay >= mid if closed else ay > mid).to(torch.uint8)
    code |= ((y < 0) & (code > 0)).to(torch.uint8) << 3
    code = code.reshape(w.shape[0], -1)
    return code[:, 0::2] | (code[:, 1::2] << 4), byte.to(torch.uint8).t().contiguous()


def dequantize_mxfp4(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """``codes [rows, K/2]`` (uint8 / int8), ``scales uint8 [K/32, rows]`` -> float64 ``[rows, K]`` (exact)."""
    c = codes.view(torch.uint8)
    nib = torch.stack((c & 15, c >> 4), dim=-1).reshape(c.shape[0], -1).long()
    val = torch.tensor(E2M1_VALUES, dtype=torch.float64, device=c.device)[nib & 7] * (1.0 - 2.0 * (nib >> 3).double())
    s = torch.ldexp(torch.ones((), dtype=torch.float64, device=c.device), scales.t().to(torch.int32) - 127)
    return (val.reshape(c.shape[0], -1, BLOCK) * s.unsqueeze(-1)).reshape(c.shape[0], -1)


def pack_scales_mxfp4(scales: torch.Tensor) -> torch.Tensor:
    """``scales uint8 [K/32, rows]`` -> the kernels' scale operand ``uint8 [K/128, rows, 4]``: the four blocks of a 128-channel K-step in one dword."""
    g, rows = scales.shape
    if g % 4:
        raise ValueError("pack_scales_mxfp4: K must be a multiple of 128")
    return scales.reshape(g // 4, 4, rows).permute(0, 2, 1).contiguous()


def unpack_scales_mxfp4(packed: torch.Tensor) -> torch.Tensor:
    """the inverse of :func:`pack_scales_mxfp4`"""
    kp, rows, _ = packed.shape
    return packed.permute(0, 2, 1).reshape(kp * 4, rows).contiguous()
