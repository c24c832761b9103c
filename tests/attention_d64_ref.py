"""fp32 restatement of ``svdq_attention_d64`` for the tests: per sample and head, ``softmax(scale * q k^T) v`` at head dimension 64 over all N
keys, no mask.  It is tests/xattn_ref.py's restatement with every sample owning the N rows of its own key buffer."""

import torch

from tests.softmax_profiles import chunked_softmax_ref
from tests.xattn_ref import sdpa16, xattn_ref

HEAD_DIM = 64


def attention_d64_ref(q, k, v, heads: int, scale=None, dtype=torch.float32):
    """q [B, T, >= H*64], k / v [B, N, H*64] (any strides) -> [B, T, H*64] in ``dtype`` (not rounded to 16 bits)"""
    B, N = k.shape[:2]
    hd = heads * HEAD_DIM
    return xattn_ref(q, k.reshape(B * N, hd), v.reshape(B * N, hd), heads, HEAD_DIM, [b * N for b in range(B)], [N] * B, scale, dtype)


def sdpa16_d64(q, k, v, heads: int, scale=None):
    """torch's own 16-bit attention on the same operands (the comparison of the accuracy gate)"""
    B, N = k.shape[:2]
    hd = heads * HEAD_DIM
    return sdpa16(q, k.reshape(B * N, hd), v.reshape(B * N, hd), heads, HEAD_DIM, [b * N for b in range(B)], [N] * B, scale)


def kernel_order_ref(q, k, v, heads: int, scale=None, dtype=torch.bfloat16):
    """The kernel's own order of operations in fp32 on the CPU: 64-key chunks from key 0, online softmax with exp2 and scale * log2(e), P rounded
    to ``dtype`` before it meets V, the row sum over the rounded values, the normalisation last.  q [T, H*64], k / v [N, H*64] -> [T, H*64] fp32
    (before the final rounding).  What this differs from the kernel in: the order of the fp32 additions inside a matrix product.
    It is tests/softmax_profiles.py's chunked_softmax_ref at head dimension 64."""
    return chunked_softmax_ref(q, k, v, heads, HEAD_DIM, scale, dtype)
