"""CPU restatements of svdq_dwconv3x3 (SANA's depthwise 3x3 convolution; include/svdq_amd.h): cross-correlation, stride 1, zero padding 1, on a
channels-last ``x [B, H, W, C]`` with the reference's ``weight [C, 3, 3, 1]`` and ``bias [C]`` (or None).

The kernel's arithmetic is specified operation by operation, so ``dwconv_ref32`` is bit-equal to it: an fp32 accumulator that starts at the bias
(or +0), the nine taps added in row-major (ky, kx) order, a tap outside the image contributing its product with a zero, one rounding to the
16-bit type at the end.  (A product of two 16-bit values is exact in fp32: a multiply followed by an add rounds where the kernel's FMA does.)"""

import torch
import torch.nn.functional as F


def _taps(x, weight, bias, dtype, round_each=None):
    B, H, W, C = x.shape
    xp = F.pad(x.to(dtype), (0, 0, 1, 1, 1, 1))             # zero rows and columns around the image
    w = weight.to(dtype).reshape(C, 3, 3)
    acc = (torch.zeros(C, dtype=dtype) if bias is None else bias.to(dtype)).expand(B, H, W, C).clone()
    for ky in range(3):
        for kx in range(3):
            acc = acc + w[:, ky, kx] * xp[:, ky:ky + H, kx:kx + W, :]
            if round_each is not None:
                acc = acc.to(round_each).to(dtype)
    return acc


def dwconv_ref32(x, weight, bias=None):
    """the kernel's arithmetic in torch fp32 on the CPU, rounded once to the dtype of ``x``: bit-equal to the kernel"""
    return _taps(x.cpu(), weight.cpu(), None if bias is None else bias.cpu(), torch.float32).to(x.dtype)


def dwconv_ref64(x, weight, bias=None):
    """the same sum in float64, not rounded"""
    return _taps(x.cpu(), weight.cpu(), None if bias is None else bias.cpu(), torch.float64)


def dwconv_16bit(x, weight, bias=None):
    """the reference's arithmetic (ElementAccumulator = half_t, src/kernels/dwconv.cu:223): the accumulator rounded to the 16-bit type after every
    tap.  For comparison only."""
    return _taps(x.cpu(), weight.cpu(), None if bias is None else bias.cpu(), torch.float32, round_each=x.dtype).to(x.dtype)


def abs_terms(x, weight, bias=None):
    """|bias| + sum |w * x| in float64: the magnitude the rounding-error bound of an fp32 sum scales with"""
    return _taps(x.cpu().abs(), weight.cpu().abs(), None if bias is None else bias.cpu().abs(), torch.float64)
