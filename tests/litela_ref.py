"""CPU restatements of SANA's ReLU linear attention for the tests (test infrastructure; plain torch ops).

Column order of the packed QKV projection (reference: epilogues.cuh:552-761, gemm_w4a4_launch_impl.cuh:311-345): the first ``H*32`` columns
are Q, head ``h`` at ``32 h``; behind them every head has 64 columns, 32 of K then 32 of V.  Per batch element and head, over the tokens:

    vk[i, j]  = sum_t V[t, i] * relu(K[t, j])        vk[32, j] = sum_t relu(K[t, j])
    out[t, i] = (sum_j relu(Q[t, j]) * vk[i, j]) / (sum_j relu(Q[t, j]) * vk[32, j] + eps)
"""
import torch

D = 32


def split_qkv(qkv: torch.Tensor, heads: int):
    """packed [B, T, 3*H*32] -> q, k, v as [B, T, H, 32] views"""
    B, T, W = qkv.shape
    assert W == 3 * heads * D
    kv = qkv[..., heads * D:].reshape(B, T, heads, 2 * D)
    return qkv[..., : heads * D].reshape(B, T, heads, D), kv[..., :D], kv[..., D:]


def _litela(q, k, v, eps):
    rq, rk = torch.relu(q), torch.relu(k)
    vk = torch.einsum("bthi,bthj->bhij", v, rk)
    ksum = rk.sum(dim=1)  # [B, H, 32]
    num = torch.einsum("bthj,bhij->bthi", rq, vk)
    den = torch.einsum("bthj,bhj->bth", rq, ksum) + eps
    out = num / den[..., None]
    return out.reshape(out.shape[0], out.shape[1], -1), torch.cat([vk, ksum[:, :, None, :]], dim=2)


def litela_ref64(qkv: torch.Tensor, heads: int, eps: float = 1e-6):
    """fp64 on the values as given: ``(out [B, T, H*32], vk [B, H, 33, 32])``, both float64, unrounded"""
    return _litela(*(t.double() for t in split_qkv(qkv.cpu(), heads)), eps)


def litela_ref32(qkv: torch.Tensor, heads: int, eps: float = 1e-6):
    """fp32 throughout, ``out`` rounded ONCE to the dtype of ``qkv``: ``(out, vk float32)``"""
    out, vk = _litela(*(t.float() for t in split_qkv(qkv.cpu(), heads)), eps)
    return out.to(qkv.dtype), vk


def litela_ones_row(qkv: torch.Tensor, heads: int, eps: float = 1e-6):
    """the same numbers from the "append a row of ones to V" formulation: one [33, 32] product per head, row 32 is the denominator's"""
    q, k, v = (t.double() for t in split_qkv(qkv.cpu(), heads))
    v1 = torch.cat([v, torch.ones_like(v[..., :1])], dim=-1)  # [B, T, H, 33]
    vk = torch.einsum("bthi,bthj->bhij", v1, torch.relu(k))
    o = torch.einsum("bthj,bhij->bthi", torch.relu(q), vk)    # [B, T, H, 33]
    out = o[..., :D] / (o[..., D:] + eps)
    return out.reshape(out.shape[0], out.shape[1], -1), vk


def litela_16bit(qkv: torch.Tensor, heads: int, eps: float = 1e-6):
    """what torch ops in the 16-bit dtype alone give (every intermediate rounded, vk in 16 bits): the comparison figure of the GPU tests"""
    out, _ = _litela(*split_qkv(qkv, heads), eps)
    return out
