"""References for ``svdq_attention_d64_bias``: its formula in float64, and transformers' eager T5 sequence (matmul, add bias, add mask, softmax, matmul) in 16 bits."""

import torch


def _dense_bias(rel_bias, key_bias, B, T, N):  # [B, H, T, N]: rel_bias[h, n - t + T - 1] + key_bias[b, n]
    idx = torch.arange(N, device=rel_bias.device)[None, :] - torch.arange(T, device=rel_bias.device)[:, None] + T - 1
    bias = rel_bias[:, idx][None].expand(B, -1, -1, -1)
    return bias if key_bias is None else bias + key_bias[:, None, None, :]


def attention_d64_bias_ref(q, k, v, heads, rel_bias, key_bias=None, scale=1.0):
    """float64 ``softmax_n(scale q.k + rel_bias + key_bias) v`` per sample and head; q [B, T, H*64], k / v [B, N, H*64] -> [B, T, H*64] float64"""
    (B, T, _), N = q.shape, k.shape[1]
    qh, kh, vh = (t.double().unflatten(-1, (heads, 64)).transpose(1, 2) for t in (q, k, v))
    s = scale * qh @ kh.transpose(2, 3) + _dense_bias(rel_bias.double(), None if key_bias is None else key_bias.double(), B, T, N)
    return (torch.softmax(s, dim=-1) @ vh).transpose(1, 2).reshape(B, T, heads * 64)


def eager16_d64_bias(q, k, v, heads, rel_bias, key_bias=None, scale=1.0):
    """transformers' eager sequence in the inputs' 16-bit dtype: the scores, the position bias and the mask are 16-bit tensors"""
    (B, T, _), N = q.shape, k.shape[1]
    qh, kh, vh = (t.unflatten(-1, (heads, 64)).transpose(1, 2) for t in (q, k, v))
    w = torch.matmul(qh, kh.transpose(2, 3)) * scale
    w = w + _dense_bias(rel_bias, None, 1, T, N).to(q.dtype)
    w = w if key_bias is None else w + key_bias.to(q.dtype)[:, None, None, :]
    w = torch.softmax(w, dim=-1)
    return torch.matmul(w, vh).transpose(1, 2).reshape(B, T, heads * 64)
