"""Activation quantiser wrapper (reference: nunchaku/ops/quantize.py:11-81)."""

from __future__ import annotations

import torch

from .._C import ops
from ..mode import alloc_lora_act
from ..utils import ceil_divide
from .conv import grid_of
from .elementwise import ln_pool


def svdq_quantize_w4a4_act_fuse_lora_cuda(
    input: torch.Tensor,
    output: torch.Tensor | None = None,
    oscales: torch.Tensor | None = None,
    lora_down: torch.Tensor | None = None,
    lora_act_out: torch.Tensor | None = None,
    smooth: torch.Tensor | None = None,
    fuse_glu: bool = False,
    fp4: bool = False,
    pad_size: int = 256,
    ln: tuple | None = None,
    pool=None,
    lora_act_zeroed: bool = False,
    second: dict | None = None,
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """4-bit quantisation of ``input`` [M, K] (``fuse_glu``: [M, 2K] interleaved (value, gate) pairs, quantised as
    ``value * silu(gate)``) plus the low-rank down projection.

    Returns ``(output [M_pad, 3K/4] uint8, oscales [K/64, M_pad], lora_act_out [M_pad, R] float32)``
    with ``M_pad = ceil(M / pad_size) * pad_size``.  ``output`` and ``oscales`` are opaque (the FP6
    operand image / scale image of this library: 6 bits per 4-bit code, so the code buffer is 1.5x the
    reference's ``[M_pad, K/2]``); ``lora_act_out`` holds the true fp32 projection.
    ``ln = (stats, scale, shift)`` (extension): quantise ``layer_norm(input) * scale + shift`` computed on
    the fly from the row statistics of ``ops.elementwise.residual_gate_stats`` -- the AdaLayerNormZero front end.
    """
    if fp4:
        raise NotImplementedError("NVFP4 is not available on MI355X")
    M, K = input.shape
    if fuse_glu:  # [M, 2K] (value, gate) pairs -> K quantised channels (the reference's wrapper sizes its buffers from the
        K //= 2   # input width and can only be called with caller-sized ones in this mode, launch_impl.cuh:463-467)
    R = lora_down.shape[1]
    M_pad = ceil_divide(M, pad_size) * pad_size
    dev = input.device
    if output is None:
        output = torch.empty(M_pad, K * 3 // 4, dtype=torch.uint8, device=dev)
    if oscales is None:
        if K % 128:
            raise ValueError("K must be a multiple of 128")
        oscales = torch.empty(K // 64, M_pad, dtype=input.dtype, device=dev)
    zeroed = bool(lora_act_zeroed)  # only meaningful with a caller-provided lora_act_out
    if lora_act_out is None:
        # a 4th element of ``ln`` is a ZeroPool of fp32 scratch cleared by the preceding residual_gate_stats pass
        if pool is None:
            pool = ln_pool(ln)
        lora_act_out, zeroed = alloc_lora_act(M_pad, R, dev, pool)  # fp32, or int64 fixed point in deterministic mode
    if ln is None:
        ops.quantize_w4a4_act_fuse_lora(input, output, oscales, lora_down, lora_act_out, smooth, fuse_glu, fp4,
                                        lora_act_zeroed=zeroed, second=second)
    else:
        ops.quantize_w4a4_act_fuse_lora(input, output, oscales, lora_down, lora_act_out, smooth, fuse_glu, fp4,
                                        ln_stats=ln[0], mod_scale=ln[1], mod_shift=ln[2], lora_act_zeroed=zeroed, second=second)
    return output, oscales, lora_act_out


def svdq_quantize_glu_halves(x: torch.Tensor, *, lora_down: torch.Tensor | None, smooth: torch.Tensor | None, act: str = "silu", pad_size: int = 256,
                             pool=None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """4-bit quantisation of ``value * act(gate)`` plus the low-rank down projection, where ``value, gate = x.chunk(2, -1)`` of a projection
    output ``x`` [N, 2K]: both halves are read in place (no chunk, no copy) and the 16-bit [N, K] product is never written.  ``act``:
    ``"silu"`` (SwiGLU) or ``"gelu"`` (GEGLU, erf form).  The 16-bit rounding points are those of the torch sequence
    ``value * act(gate)``; returns what :func:`svdq_quantize_w4a4_act_fuse_lora_cuda` returns for that product."""
    if x.dim() != 2 or x.shape[1] % 2:
        raise ValueError("svdq_quantize_glu_halves: x must be [N, 2K]")
    if x.stride(1) != 1:
        x = x.contiguous()
    M, K = x.shape[0], x.shape[1] // 2
    if K % 128:
        raise ValueError("K must be a multiple of 128")
    R = 0 if lora_down is None else lora_down.shape[1]
    M_pad = ceil_divide(M, pad_size) * pad_size
    output = torch.empty(M_pad, K * 3 // 4, dtype=torch.uint8, device=x.device)
    oscales = torch.empty(K // 64, M_pad, dtype=x.dtype, device=x.device)
    lora_act_out, zeroed = alloc_lora_act(M_pad, R, x.device, pool)
    ops.quantize_glu_halves(x, output, oscales, lora_down, lora_act_out, smooth, act=act, lora_act_zeroed=zeroed)
    return output, oscales, lora_act_out


def svdq_quantize_dwconv_glu(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, height: int | None = None, width: int | None = None,
                             lora_down: torch.Tensor | None = None, smooth: torch.Tensor | None = None, quantized_features: int | None = None,
                             pad_size: int = 256, pool=None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The back half of SANA's GLU-MBConv in one launch (``svdq_quantize_dwconv_glu``): ``c = dwconv3x3(x, weight, bias)`` in that kernel's
    arithmetic, ``value, gate = c[..., 0::2], c[..., 1::2]``, then the 4-bit quantisation of ``value * silu(gate)`` plus the low-rank down
    projection -- what ``dwconv3x3`` followed by :func:`svdq_quantize_w4a4_act_fuse_lora_cuda` ``(fuse_glu=True)`` computes, without the 16-bit
    convolution output in between.  ``x``: ``[B, H, W, C]``, or ``[B, T, C]`` with ``height`` / ``width`` (as for ``dwconv3x3``; it may be a
    column slice of a wider buffer); ``weight``: ``[C, 3, 3, 1]``, ``bias``: ``[C]`` or None.  ``quantized_features`` ``K`` (default ``C / 2``):
    the quantised width, a multiple of 128 with ``C <= 2K`` -- the conv channels behind ``C`` count as zeros and are not read.  Row
    ``b * H * W + h * W + w`` of the result is pixel ``(b, h, w)``; returns ``(qx, ascales, lora_act)`` as the other quantisers do."""
    if x.dim() == 4:
        B, H, W, C = x.shape
        if (height is not None and int(height) != H) or (width is not None and int(width) != W):
            raise ValueError(f"svdq_quantize_dwconv_glu: height / width ({height}, {width}) contradict x {tuple(x.shape)}")
        x4 = x
    elif x.dim() == 3:
        B, T, C = x.shape
        H, W = grid_of(T, height, width)
        x4 = x.unflatten(1, (H, W))
    else:
        raise ValueError("svdq_quantize_dwconv_glu: expected x [B, H, W, C], or [B, T, C] with height / width")
    K = C // 2 if quantized_features is None else int(quantized_features)
    if K < 1 or K % 128 or C > 2 * K:
        raise ValueError(f"svdq_quantize_dwconv_glu: the quantised width {K} must be a multiple of 128 with C={C} <= 2K")
    R = 0 if lora_down is None else lora_down.shape[1]
    M_pad = ceil_divide(B * H * W, pad_size) * pad_size
    output = torch.empty(M_pad, K * 3 // 4, dtype=torch.uint8, device=x.device)
    oscales = torch.empty(K // 64, M_pad, dtype=x.dtype, device=x.device)
    lora_act_out, zeroed = alloc_lora_act(M_pad, R, x.device, pool)
    ops.quantize_dwconv_glu(x4, weight, bias, output, oscales, lora_down, lora_act_out, smooth, lora_act_zeroed=zeroed)
    return output, oscales, lora_act_out


def svdq_quantize_mxfp4(x: torch.Tensor, lora_down: torch.Tensor | None = None, smooth: torch.Tensor | None = None,
                        pad_size: int = 256) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """OCP MXFP4 quantisation of ``x`` [M, K] (after the smoothing division) plus the low-rank down projection ``x @ lora_down`` (``lora_down``:
    the logical ``[K, R]`` factor).  Returns ``(act uint8 [M_pad, K/2]`` e2m1 codes in natural rows, ``ascales uint8 [K/128, M_pad, 4]`` E8M0 bytes
    with the four 32-channel blocks of a K-step in one dword, ``lora_act float32 [M_pad, R])``; rows from M on are zeros.
    ``quantization.mxfp4.unpack_scales_mxfp4`` turns ``ascales`` into ``[K/32, M_pad]``."""
    if x.dim() != 2:
        raise ValueError("svdq_quantize_mxfp4: x must be [M, K]")
    if x.stride(1) != 1:
        x = x.contiguous()
    M, K = x.shape
    if K % 128:
        raise ValueError(f"svdq_quantize_mxfp4: K={K} must be a multiple of 128")
    if pad_size < 1 or pad_size % 256:
        raise ValueError("svdq_quantize_mxfp4: pad_size must be a multiple of 256")
    R = 0 if lora_down is None else lora_down.shape[1]
    M_pad = ceil_divide(M, pad_size) * pad_size
    act = torch.empty(M_pad, K // 2, dtype=torch.uint8, device=x.device)
    ascales = torch.empty(K // 128, M_pad, 4, dtype=torch.uint8, device=x.device)
    lora_act = torch.empty(M_pad, R, dtype=torch.float32, device=x.device)
    ops.quantize_mxfp4(x, act, ascales, lora_down, lora_act, smooth)
    return act, ascales, lora_act
