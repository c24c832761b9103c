"""fp32 restatement of ``svdq_attention_d64`` for the tests: per sample and head, ``softmax(scale * q k^T) v`` at head dimension 64 over all N
keys, no mask.  It is tests/xattn_ref.py's restatement with every sample owning the N rows of its own key buffer."""

import torch

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
    (before the final rounding).  What this differs from the kernel in: the order of the fp32 additions inside a matrix product."""
    T, N = q.shape[0], k.shape[0]
    c = (HEAD_DIM ** -0.5 if scale is None else scale) * 1.4426950408889634
    qh = q.float().view(T, heads, HEAD_DIM).transpose(0, 1)
    kh = k.float().view(N, heads, HEAD_DIM).transpose(0, 1)
    vh = v.float().view(N, heads, HEAD_DIM).transpose(0, 1)
    m = torch.full((heads, T, 1), float("-inf"))
    l = torch.zeros(heads, T, 1)
    o = torch.zeros(heads, T, HEAD_DIM)
    for n0 in range(0, N, 64):
        s = qh @ kh[:, n0:n0 + 64].transpose(1, 2)
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp2((m - m_new) * c)
        p = torch.exp2(s * c - m_new * c).to(dtype).float()
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p @ vh[:, n0:n0 + 64]
        m = m_new
    return (o / l).transpose(0, 1).reshape(T, heads * HEAD_DIM)
