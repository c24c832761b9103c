"""Reference of ``ops.quantize.svdq_quantize_dwconv_glu``: the convolution bit-equal on the CPU (tests/dwconv_ref.py), the conv channels behind ``C``
as zeros, the interleaved pairs de-interleaved, then tests/glu_halves_ref.py (float64 activation and product, the oracle's quantiser)."""

import numpy as np

from tests.dwconv_ref import dwconv_ref32
from tests.glu_halves_ref import glu_halves, quantize_glu_halves
from tests.helpers import f32


def conv_pairs(x, weight, bias, K):  # x [B, H, W, C] 16-bit torch -> (value, gate) [B * H * W, K] float32
    c = f32(dwconv_ref32(x, weight, bias)).reshape(-1, x.shape[-1])
    c = np.concatenate([c, np.zeros((c.shape[0], 2 * K - c.shape[1]), np.float32)], axis=1)
    return np.ascontiguousarray(c[:, 0::2]), np.ascontiguousarray(c[:, 1::2])


def quantize_dwconv_glu(x, weight, bias, smooth, lora_down, K, dtype):  # -> (codes, ascales, lora_act | None), the 16-bit product [M, K]
    value, gate = conv_pairs(x, weight, bias, K)
    return quantize_glu_halves(value, gate, smooth, lora_down, dtype, "silu"), glu_halves(value, gate, dtype, "silu")
