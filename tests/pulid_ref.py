"""CPU restatements for the PuLID tests (test infrastructure): the float64 reference composition and its folded evaluation, and the
arithmetic contract of ``svdq_pulid_ca`` behind its two MFMA accumulators, operation by operation (include/svdq_amd.h,
nunchaku_amd/csrc/pulid_ca.hip).  The order in which the matrix core sums an accumulator's terms is not restated: the bit-exact functions
here start from an accumulator (``probs_from_acc``, ``out_from_o``); ``kernel_ref`` forms the accumulators with fp32 matrix products."""
import copy
import math

import torch
import torch.nn.functional as F

from nunchaku_amd.models.pulid import FOLD_TOKENS, PerceiverAttentionCA, fold_terms

TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
EXP_FLOOR = -80.0


def module_state_dict(count: int, dim: int, heads: int, kv_dim: int, dim_head: int = 128, seed: int = 0, dtype=torch.bfloat16,
                      out_scale: float = 1.0, encoder: bool = True) -> dict:
    """A synthetic PuLID file's content with the reference's key names: ``pulid_ca.<k>.*`` and a few ``pulid_encoder.*`` tensors"""
    g = torch.Generator().manual_seed(seed)
    inner = heads * dim_head
    r = lambda *shape: torch.randn(*shape, generator=g)
    sd = {}
    for k in range(count):
        p = f"pulid_ca.{k}."
        sd[p + "norm1.weight"], sd[p + "norm1.bias"] = (1 + 0.2 * r(kv_dim)).to(dtype), (0.1 * r(kv_dim)).to(dtype)
        sd[p + "norm2.weight"], sd[p + "norm2.bias"] = (1 + 0.2 * r(dim)).to(dtype), (0.1 * r(dim)).to(dtype)
        sd[p + "to_q.weight"] = (r(inner, dim) / dim ** 0.5).to(dtype)
        sd[p + "to_kv.weight"] = (r(2 * inner, kv_dim) / kv_dim ** 0.5).to(dtype)
        sd[p + "to_out.weight"] = (r(dim, inner) * (out_scale / inner ** 0.5)).to(dtype)
    if encoder:
        sd["pulid_encoder.latents"] = torch.zeros(1, 4, 8, dtype=dtype)
        sd["pulid_encoder.proj_out"] = torch.zeros(8, 8, dtype=dtype)
    return sd


def make_module(dim: int, heads: int, kv_dim: int, dim_head: int, seed: int = 0, dtype=torch.bfloat16, device="cpu") -> PerceiverAttentionCA:
    m = PerceiverAttentionCA(dim=dim, dim_head=dim_head, heads=heads, kv_dim=kv_dim, dtype=dtype, device=device)
    sd = module_state_dict(1, dim, heads, kv_dim, dim_head, seed=seed, dtype=dtype, encoder=False)
    m.load_state_dict({k[len("pulid_ca.0."):]: v for k, v in sd.items()}, strict=True)
    return m


def compose64(mod: PerceiverAttentionCA, x: torch.Tensor, latents: torch.Tensor) -> torch.Tensor:
    """the reference's torch-op sequence on the module's (16-bit) parameter values, in float64: ``[T, dim]``.  (Restated, not
    ``mod.forward``: that casts the scores to float32 for the softmax, as the reference does.)"""
    m64 = copy.deepcopy(mod).double().cpu()
    x2, lat = x.double().cpu().reshape(-1, x.shape[-1]), latents.double().cpu().reshape(-1, latents.shape[-1])
    h = m64.heads
    q = m64.to_q(m64.norm2(lat)).view(lat.shape[0], h, -1).transpose(0, 1)
    k, v = (t.reshape(x2.shape[0], h, -1).transpose(0, 1) for t in m64.to_kv(m64.norm1(x2)).chunk(2, dim=-1))
    scale = 1 / math.sqrt(math.sqrt(m64.dim_head))
    weight = torch.softmax((q * scale) @ (k * scale).transpose(-2, -1), dim=-1)
    return m64.to_out((weight @ v).transpose(0, 1).reshape(lat.shape[0], -1))


def folded64(mod: PerceiverAttentionCA, x: torch.Tensor, latents: torch.Tensor) -> torch.Tensor:
    """the folded evaluation with no rounding anywhere, in float64: ``softmax(LN(latents) . a_h^T + cbias_h) . b_h`` summed over heads"""
    m64 = copy.deepcopy(mod).double().cpu()
    x2, lat = x.double().cpu().reshape(-1, x.shape[-1]), latents.double().cpu().reshape(-1, latents.shape[-1])
    k, v = m64.to_kv(m64.norm1(x2)).chunk(2, dim=-1)
    a, cb, b = fold_terms(k, v, m64.to_q.weight, m64.to_out.weight, m64.norm2.weight, m64.norm2.bias, m64.heads)
    n = F.layer_norm(lat, (lat.shape[-1],), eps=m64.norm2.eps)
    s = torch.einsum("tc,hnc->thn", n, a) + cb[None]
    return torch.einsum("thn,hnc->tc", torch.softmax(s, dim=-1), b)


def row_stats(x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """``[T, 2]`` float32 (mean, rstd) of the rows of a 16-bit ``x``, two passes in fp32"""
    xf = x.float().cpu()
    mean = xf.mean(dim=-1, keepdim=True)
    var = ((xf - mean) ** 2).mean(dim=-1, keepdim=True)
    return torch.cat([mean, 1.0 / torch.sqrt(var + eps)], dim=-1)


def exp_ref(d0: torch.Tensor) -> torch.Tensor:
    """``pulid_exp``: exp(d) for d <= 0 from fp32 operations, one rounding each (float32 CPU tensor in, float32 out)"""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    d = torch.maximum(d0, f(-100.0))
    t = d * f(1.4426950408889634)
    n = torch.round(t)  # half to even, as v_rndne_f32
    r = d - n * f(0.693145751953125)
    r = r - n * f(1.428606765330187e-06)
    p = f(1.0) / f(5040.0)
    for c in (f(1.0) / f(720.0), f(1.0) / f(120.0), f(1.0) / f(24.0), f(1.0) / f(6.0), f(0.5), f(1.0), f(1.0)):
        p = p * r
        p = p + c
    e = (p.contiguous().view(torch.int32) + n.to(torch.int32) * (1 << 23)).view(torch.float32)
    return torch.where(d < EXP_FLOOR, torch.zeros_like(e), e)


def probs_from_acc(acc: torch.Tensor, stats: torch.Tensor, colsum: torch.Tensor, cbias: torch.Tensor, tokens: int, dtype) -> torch.Tensor:
    """The score epilogue, bit for bit: ``acc`` ``[T, H * 32]`` float32 (the kernel's accumulator) -> the 16-bit probabilities.
    ``s = rstd (acc - mean colsum) + cbias``; keys ``n >= tokens`` are -inf; ``e = exp(s - max)``; the sum runs as the kernel's lanes hold
    the keys -- lane half ``h`` owns the keys ``8 g + 4 h + e`` (g, e < 4) and adds them in that order, then the two halves are added --
    and ``P = round16(e / sum)`` with an IEEE division."""
    acc, stats, colsum, cbias = (t.detach().float().cpu() for t in (acc, stats, colsum, cbias))
    T, J = acc.shape
    H = J // FOLD_TOKENS
    mean, rstd = stats[:, 0:1], stats[:, 1:2]
    mc = mean * colsum[None]
    d = acc - mc
    sd = rstd * d
    s = (sd + cbias[None]).view(T, H, FOLD_TOKENS)
    s = torch.where(torch.arange(FOLD_TOKENS)[None, None] < tokens, s, torch.full_like(s, float("-inf")))
    m = s.max(dim=-1, keepdim=True).values
    e = exp_ref(s - m)
    lanes = e.view(T, H, 4, 2, 4).permute(0, 1, 3, 2, 4).reshape(T, H, 2, 16)  # [.., lane half, register]
    half = torch.zeros(T, H, 2, dtype=torch.float32)
    for r in range(16):
        half = half + lanes[..., r]
    total = (half[..., 0] + half[..., 1])[..., None]
    return (e / total).to(dtype).view(T, J)


def out_from_o(o: torch.Tensor, out_scale: float, dtype) -> torch.Tensor:
    """The output epilogue, bit for bit: ``round16(out_scale * round16(o))``, the product in fp32 with the fp32 scale"""
    o16 = o.detach().float().cpu().to(dtype).float()
    return (o16 * torch.tensor(out_scale, dtype=torch.float32)).to(dtype)


def kernel_ref(x: torch.Tensor, fold, out_scale: float = 1.0, stats: torch.Tensor | None = None):
    """The kernel's rounding points on the CPU with fp32 matrix products for the two accumulators: ``(out, probs)`` 16-bit"""
    dtype = x.dtype
    xf = x.float().cpu()
    stats = row_stats(x) if stats is None else stats
    acc = xf @ fold.a_fold.float().cpu().T
    probs = probs_from_acc(acc, stats, fold.colsum, fold.cbias, fold.tokens, dtype)
    o = probs.float() @ fold.b_fold.float().cpu()
    return out_from_o(o, out_scale, dtype), probs


def stream_inputs(T: int, C: int, seed: int, dtype, device="cpu", ld: int | None = None) -> torch.Tensor:
    """An image stream that exercises the mean subtraction: per-row mean 8, std 1, one outlier channel of 200 -- ``[T, C]``, as the first
    ``C`` columns of ``[T, ld]`` rows when ``ld`` is given"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, C, generator=g) + 8.0
    x[:, (7 * seed + 3) % C] = 200.0
    x = x.to(dtype)
    if ld is None:
        return x.to(device)
    buf = torch.full((T, ld), float("nan"), dtype=dtype)
    buf[:, :C] = x
    return buf.to(device)[:, :C]
