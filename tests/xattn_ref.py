"""fp32 restatement of SANA's cross-attention for the tests: per sample and head, ``softmax(scale * q k^T) v`` over the sample's key range,
zeros for an empty range.  Ranges are host integers here (the restatement is the yardstick, not the sync-free path)."""

import torch


def clamp_ranges(offsets, counts, nrows: int, max_keys: int):
    """what svdq_cross_attention makes of the ranges it reads: count to [0, max_keys], an offset outside [0, nrows) empties the range, the
    range is cut at nrows"""
    out = []
    for off, n in zip(offsets, counts):
        n = min(max(int(n), 0), max_keys)
        off = int(off)
        if off < 0 or off >= nrows:
            n = 0
        out.append((off, min(n, max(nrows - off, 0))))
    return out


def xattn_ref(q, k, v, heads: int, head_dim: int, offsets, counts, scale=None, dtype=torch.float32):
    """q [B, T, >= H*D], k / v [Nrows, H*D]; offsets / counts: sequences of B ints -> [B, T, H*D] in ``dtype`` (not rounded to 16 bits)"""
    B, T = q.shape[:2]
    hd = heads * head_dim
    scale = head_dim ** -0.5 if scale is None else scale
    out = torch.zeros(B, T, hd, dtype=dtype, device=q.device)
    for b, (off, n) in enumerate(zip(offsets, counts)):
        if n <= 0:
            continue
        qb = q[b, :, :hd].to(dtype).view(T, heads, head_dim).transpose(0, 1)              # [H, T, D]
        kb = k[off:off + n].to(dtype).view(n, heads, head_dim).transpose(0, 1)            # [H, n, D]
        vb = v[off:off + n].to(dtype).view(n, heads, head_dim).transpose(0, 1)
        p = torch.softmax(scale * (qb @ kb.transpose(1, 2)), dim=-1)
        out[b] = (p @ vb).transpose(0, 1).reshape(T, hd)
    return out


def sdpa16(q, k, v, heads: int, head_dim: int, offsets, counts, scale=None):
    """torch's own 16-bit attention per sample on the sliced keys (the comparison of the accuracy gate and of the benchmark)"""
    B, T = q.shape[:2]
    hd = heads * head_dim
    out = torch.zeros(B, T, hd, dtype=q.dtype, device=q.device)
    for b, (off, n) in enumerate(zip(offsets, counts)):
        if n <= 0:
            continue
        qb = q[b, :, :hd].reshape(1, T, heads, head_dim).transpose(1, 2)
        kb = k[off:off + n].reshape(1, n, heads, head_dim).transpose(1, 2)
        vb = v[off:off + n].reshape(1, n, heads, head_dim).transpose(1, 2)
        out[b] = torch.nn.functional.scaled_dot_product_attention(qb, kb, vb, scale=scale).transpose(1, 2).reshape(T, hd)
    return out
