"""Depthwise 3x3 convolution of SANA's GLU-MBConv (reference: ``DWCONV``, src/Linear.cpp:542-551 -> ``dwconv_f16``, src/kernels/dwconv.cu)."""

from __future__ import annotations

import math

import torch

from .._C import ops


def grid_of(tokens: int, height: int | None = None, width: int | None = None) -> tuple[int, int]:
    """The (H, W) of a ``[B, T, C]`` activation, by the reference's rule (``SanaGLUMBConv::forward``, src/SanaModel.cpp:201-204): without the
    pair the grid is square, one missing side is derived from the other; ``H * W != T`` raises."""
    H = int(height) if height is not None and int(height) > 0 else None
    W = int(width) if width is not None and int(width) > 0 else None
    if H is None and W is None:
        H = W = math.isqrt(tokens)
    elif H is None:
        H = tokens // W
    elif W is None:
        W = tokens // H
    if H < 1 or W < 1 or H * W != tokens:
        raise ValueError(f"dwconv3x3: a grid of height {H} and width {W} does not hold {tokens} tokens")
    return H, W


def dwconv3x3(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, height: int | None = None, width: int | None = None,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """Depthwise 3x3 cross-correlation, stride 1, zero padding 1, over the token grid of a channels-last activation (``svdq_dwconv3x3``):
    ``out = round16(bias + sum_ky sum_kx weight[c, ky, kx] * x[h + ky - 1, w + kx - 1, c])`` -- fp32, the nine taps added in row-major order,
    rounded once (the reference rounds its 16-bit accumulator after every tap).  ``x``: ``[B, H, W, C]``, or ``[B, T, C]`` with ``height`` /
    ``width`` (a missing pair: a square grid; one missing side is derived; ``H * W != T`` raises); any row and batch stride that keeps rows
    16-byte aligned, so the input may be a column slice of a wider buffer, and so may ``out``.  ``weight``: ``[C, 3, 3, 1]``, ``bias``: ``[C]`` or
    None, in the dtype of ``x``; ``C`` a multiple of 8.  Returns ``out`` (allocated in the shape of ``x`` when not given; in place is refused).
    One launch, no atomics: bit-equal from call to call."""
    if x.dim() == 4:
        B, H, W, C = x.shape
        if (height is not None and int(height) != H) or (width is not None and int(width) != W):
            raise ValueError(f"dwconv3x3: height / width ({height}, {width}) contradict x {tuple(x.shape)}")
        x4 = x
    elif x.dim() == 3:
        B, T, C = x.shape
        H, W = grid_of(T, height, width)
        x4 = x.unflatten(1, (H, W))
    else:
        raise ValueError("dwconv3x3: expected x [B, H, W, C], or [B, T, C] with height / width")
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    if tuple(out.shape) not in ((B, H, W, C), (B, H * W, C)):
        raise ValueError(f"dwconv3x3: out must be [B, H, W, C] or [B, H * W, C] = {(B, H, W, C)}, got {tuple(out.shape)}")
    ops.dwconv3x3(x4, weight, bias, out if out.dim() == 4 else out.unflatten(1, (H, W)))
    return out
