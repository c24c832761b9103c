"""What the FLUX joint block (models/flux.py) and the Qwen-Image block (models/qwenimage.py) share.  On the fused path the two are ONE
computation, written out here once (:func:`joint_attention`, :func:`dual_stream_block`): grouped QKV quantiser + GEMM with the
RMSNorm + RoPE epilogue, attention with the quantising epilogue, grouped output projections, a gated-residual pass, grouped fc1
(GELU_QUANT) / fc2, a second gated-residual pass.  Around it: the feed-forward holder, the ControlNet residual, the
AdaLayerNormContinuous head, the synthetic initialiser.  What differs between the models is an argument; each model's reference-op
path stays in its own file (they restate different reference files).  Imports ``..ops`` and ``.linear`` only: no cycle."""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from ..ops.attention import alloc_qkv, attention_packed, attention_packed_quantized, q_prescale
from ..ops.elementwise import ln_pool, residual_gate_stats, residual_gate_stats_pair
from ..ops.fused import fused_gelu_mlp, fused_gelu_mlp_pair, fused_qkv_norm_rottary_pair, linear_pair, linear_pair_quantized
from .linear import AWQW4A16Linear, SVDQW4A4Linear, synthetic_codes_


def pad256(n: int) -> int:
    return (n + 255) // 256 * 256


def pair_compatible(la, lb) -> bool:
    """two projections that one grouped GEMM launch can serve (same shapes, rank, bias presence and LoRA strengths)"""
    return (la.in_features == lb.in_features and la.out_features == lb.out_features and la.rank == lb.rank
            and (la.bias is None) == (lb.bias is None) and getattr(la, "lora_scales", None) == getattr(lb, "lora_scales", None))


class _GELUProj(nn.Module):
    """``net.0`` of a diffusers FeedForward(activation_fn="gelu-approximate"): holds ``proj``; the activation itself runs in
    the projection's GEMM epilogue."""

    def __init__(self, dim, hidden, kw):
        super().__init__()
        self.proj = SVDQW4A4Linear(dim, hidden, **kw)


class FeedForward(nn.Module):
    """fc1 -> GELU(tanh) -> fc2 with the requantisation fused into fc1's epilogue (reference: NunchakuFeedForward,
    models/attention.py:76-123).  Module names are diffusers' ``net = [GELU(proj), Dropout, Linear]``: checkpoint keys
    ``<name>.net.0.proj.*`` / ``<name>.net.2.*``."""

    def __init__(self, dim, kw, mult: int = 4):
        super().__init__()
        self.net = nn.ModuleList([_GELUProj(dim, mult * dim, kw), nn.Identity(), SVDQW4A4Linear(mult * dim, dim, **{**kw, "act_unsigned": True})])

    @property
    def fc1(self) -> SVDQW4A4Linear:
        return self.net[0].proj

    @property
    def fc2(self) -> SVDQW4A4Linear:
        return self.net[2]

    def forward(self, x, ln=None):
        return fused_gelu_mlp(x, self.fc1, self.fc2, ln=ln)


def add_control(stream, samples, i: int, n_blocks: int, repeat: bool = False, want_stats: bool = True):
    """``stream += sample`` (one 16-bit add, in place) with diffusers' choice of the ControlNet residual behind block ``i`` of
    ``n_blocks`` -- ``samples[i % n]`` with ``repeat``, else ``samples[i // ceil(n_blocks / n)]`` -- in the stream's dtype, the stream's
    padded rows getting a zero residual.  ``want_stats`` (the fused path): the LayerNorm statistics of the sum come out of the same
    pass.  -> (stream, stats or None)"""
    n = len(samples)
    smp = (samples[i % n] if repeat else samples[i // -(-n_blocks // n)]).to(stream.dtype)
    if smp.shape[1] != stream.shape[1]:
        smp = F.pad(smp, (0, 0, 0, stream.shape[1] - smp.shape[1]))
    return residual_gate_stats(stream, smp, want_stats=want_stats)


class AdaLNContinuous(nn.Module):
    """diffusers' AdaLayerNormContinuous of the output head: ``linear`` (dim -> 2 dim, on the activated embedding); the LayerNorm has no
    parameters."""

    def __init__(self, dim, dtype, device):
        super().__init__()
        self.linear = nn.Linear(dim, 2 * dim, dtype=dtype, device=device)

    def forward(self, hidden, temb_act):
        scale, shift = self.linear(temb_act).chunk(2, dim=-1)
        return F.layer_norm(hidden, (hidden.shape[-1],), eps=1e-6) * (1 + scale[:, None]) + shift[:, None]


@torch.no_grad()
def init_synthetic_(model, seed: int = 0, codes: str = "uniform", repack: bool = False, awq_scale_one: bool = False,
                    linear_divides: bool = False):
    """Random weights in the checkpoint layout (no checkpoints are at hand): int4 codes uniform or distributed like a quantised Gaussian
    residual (``codes``: models/linear.py ``synthetic_codes_``), scales / low-rank factors small so that activations stay O(1).  One
    generator, the draws in module order: a seed names one set of weights.  ``repack``: into the kernel layout at once.
    ``awq_scale_one``: the modulation bias carries the +1 of every scale (nunchaku's FLUX checkpoints: scale_shift = 0,
    normalization.py:24-25).  ``linear_divides``: a dense weight is ``randn / sqrt(K)``, not ``randn * (1 / sqrt(K))`` -- one rounding
    apart; each model keeps the weights its seeds have always named."""
    dev = model.proj_out.weight.device
    g = torch.Generator(device=dev).manual_seed(seed)

    def rnd(shape, scale):
        return torch.randn(shape, generator=g, device=dev) * scale

    def uni(shape):
        return torch.rand(shape, generator=g, device=dev)

    for m in model.modules():
        if isinstance(m, SVDQW4A4Linear):
            K = m.in_features
            synthetic_codes_(m.qweight, m.wscales, K, g, codes)  # scaled so that |W row| ~ 1/sqrt(K)
            if m.bias is not None:
                m.bias.copy_(rnd(m.bias.shape, 0.02))
            m.smooth_factor.copy_(uni((K,)) + 0.5)
            m.smooth_factor_orig.copy_(m.smooth_factor)
            m.proj_down.copy_(rnd(m.proj_down.shape, 0.5 / math.sqrt(K)))
            m.proj_up.copy_(rnd(m.proj_up.shape, 0.5 / math.sqrt(m.rank)))
            m._amd_layout = False
            if repack:  # False: stay in the checkpoint layout (repacked lazily on first use, like a loaded checkpoint)
                m.repack_()
        elif isinstance(m, AWQW4A16Linear):
            # uniform 4-bit codes (std 4.6) centred by the zero point: weights ~ 1/sqrt(K)
            sc = 1.0 / (4.6 * math.sqrt(m.in_features))
            m.qweight.copy_(torch.randint(-2 ** 31, 2 ** 31, m.qweight.shape, generator=g, device=dev, dtype=torch.int64))
            m.wscales.copy_((uni(m.wscales.shape) * 0.5 + 0.75) * sc)
            m.wzeros.copy_(m.wscales.float() * -7.5)
            m.bias.zero_()
            if awq_scale_one:  # chunks (shift, SCALE, gate[, shift, SCALE, gate]) are interleaved per channel in the checkpoint's order
                m.bias.view(-1, m.out_features // m.in_features)[:, 1::3] = 1.0  # (out_chunks only permutes the OUTPUT)
        elif isinstance(m, nn.Linear):
            w = torch.randn(m.weight.shape, generator=g, device=dev)
            m.weight.copy_(w / math.sqrt(m.in_features) if linear_divides else w * (1.0 / math.sqrt(m.in_features)))
            m.bias.zero_()
        elif isinstance(m, nn.RMSNorm):
            m.weight.fill_(1.0)
    return model


def joint_attention(attn, hidden, enc, rot_all, ln=None, ln_ctx=None, kv_valid=None, quantized: bool = True):
    """Joint attention with both streams in every launch (B = 1, rows: text, then image; token counts multiples of 256): grouped QKV
    projections with the RMSNorm + RoPE epilogue into one [text; image] buffer, then :func:`joint_attention_out`.  ``attn`` exposes
    ``to_qkv / add_qkv_proj / norm_q / norm_k / norm_added_q / norm_added_k / to_add_out / to_out[0]``.  With ``ln`` / ``ln_ctx`` =
    ``(stats, scale incl. +1, shift[, ZeroPool])`` the streams come UN-normalised: AdaLayerNormZero runs inside the quantiser.
    ``rot_all``: the packed rotary table of the joint sequence.  -> (image output, text output), or None -- nothing launched --
    when the two QKV projections cannot share a launch (shapes / ranks differ)."""
    t_txt = enc.shape[1]
    qkv, vt = alloc_qkv(t_txt + hidden.shape[1], attn.heads, hidden.dtype, hidden.device, attn.head_dim)
    # Q leaves the QKV GEMM times scale * log2(e): the attention kernel's fast geometry
    if not fused_qkv_norm_rottary_pair(enc, attn.add_qkv_proj, attn.norm_added_q, attn.norm_added_k, hidden, attn.to_qkv, attn.norm_q,
                                       attn.norm_k, rot_all, qkv, out_vt=vt, ln_a=ln_ctx, ln_b=ln, q_scale=q_prescale(attn.head_dim)):
        return None
    return joint_attention_out(attn, qkv, vt, t_txt, ln_pool(ln_ctx), kv_valid, quantized)  # the pool of the stream whose rows come first


def joint_attention_out(attn, qkv, vt, t_txt: int, pool=None, kv_valid=None, quantized: bool = True):
    """Attention on the packed [text; image] buffer (Q prescaled) and the two output projections in one launch each: the attention
    epilogue emits the projections' quantised input -- the 16-bit attention output never exists.  Where that quantiser declines
    (``quantized`` off, projections that differ in shape / rank / LoRA strengths, text rows no multiple of 256) the 16-bit round trip,
    whose attention launch clears the low-rank accumulators of the projections' quantisers.  -> (image output, text output)"""
    out, add_out = attn.to_out[0], attn.to_add_out
    if quantized and pair_compatible(add_out, out):
        qres = attention_packed_quantized(qkv, vt, attn.heads, out, lin_first=add_out, split_rows=t_txt, pool=pool, q_prescaled=True,
                                          kv_valid=kv_valid)
        if qres is not None:
            ca, a = linear_pair_quantized(*qres, add_out, out, t_txt)
            return a, ca
    zf = pad256(qkv.shape[0] - t_txt) * out.rank + pad256(t_txt) * add_out.rank
    o, pool = attention_packed(qkv, vt, attn.heads, zero_floats=zf, q_prescaled=True, kv_valid=kv_valid)
    ca, a = linear_pair(o[None, :t_txt], add_out, o[None, t_txt:], out, pool=pool)
    return a, ca


def dual_stream_block(attention, attn, ff, ff_ctx, hidden, enc, stats, mod, mod_ctx, clamp_img: bool, keep_input: bool = False,
                      grouped: bool = True):
    """A dual-stream block on the fused passes (B = 1): attention, gated residual, MLP, gated residual.  LayerNorm + modulation run
    inside the quantisers; each gated residual delivers the next LayerNorm's statistics and the zeroed low-rank accumulators of the
    launches behind it in the same element-wise pass, both streams per launch.  ``attention(hidden, enc, ln, ln_ctx)`` -> (image,
    text) outputs.  ``mod`` / ``mod_ctx``: the image / text modulation as ``[6, dim]`` rows shift1, scale1, gate1, shift2, scale2,
    gate2 (scales with their +1).  ``stats`` = ((image statistics, ZeroPool or None), (text statistics, ZeroPool or None)).  An fp16
    block clips its text stream at the end; ``clamp_img``: the image stream too (Qwen-Image does, FLUX does not).  ``keep_input``: the
    first residual pass writes new tensors instead of updating the streams in place (same launches).  Text rows no multiple of 256,
    or ``grouped`` off: every stream runs its own launches.  -> (enc, hidden, stats of the outputs)"""
    (h_stats, h_pool), (e_stats, e_pool) = stats  # pools: fp32 zeros for the low-rank accumulators of the next calls
    shift1, scale1, gate1, shift2, scale2, gate2 = mod.view(6, -1)
    c_shift1, c_scale1, c_gate1, c_shift2, c_scale2, c_gate2 = mod_ctx.view(6, -1)
    a, ca = attention(hidden, enc, (h_stats, scale1, shift1, h_pool), (e_stats, c_scale1, c_shift1, e_pool))
    mp_h, mp_e = pad256(hidden.shape[1]), pad256(enc.shape[1])
    r_mlp = ff.fc1.rank + ff.fc2.rank  # fc1's quantiser + the GELU epilogue's accumulator for fc2
    if grouped and enc.shape[1] % 256 == 0:
        # grouped launches: the text stream's pool carries the scratch of BOTH streams (its rows come first)
        enc, e_stats, hidden, h_stats, e_pool = residual_gate_stats_pair(
            enc, ca, c_gate1, hidden, a, gate1, zero_floats=(mp_e + mp_h) * r_mlp, inplace=not keep_input)
        f_ctx, f = fused_gelu_mlp_pair(enc, ff_ctx.fc1, ff_ctx.fc2, hidden, ff.fc1, ff.fc2,
                                       ln_a=(e_stats, c_scale2, c_shift2, e_pool), ln_b=(h_stats, scale2, shift2))
        enc, e_stats, hidden, h_stats, e_pool = residual_gate_stats_pair(  # the accumulators of the next block's QKV + out projections
            enc, f_ctx, c_gate2, hidden, f, gate2, zero_floats=(mp_e + mp_h) * (attn.to_qkv.rank + attn.to_out[0].rank),
            clamp_fp16_a=True, clamp_fp16_b=clamp_img)
        return enc, hidden, ((h_stats, None), (e_stats, e_pool))
    hidden, h_stats, h_pool = residual_gate_stats(hidden, a, gate1, zero_floats=mp_h * r_mlp, inplace=not keep_input)
    hidden, h_stats, h_pool = residual_gate_stats(hidden, ff(hidden, ln=(h_stats, scale2, shift2, h_pool)), gate2,
                                                  zero_floats=mp_h * attn.to_qkv.rank, clamp_fp16=clamp_img)  # next block's QKV quantiser
    enc, e_stats, e_pool = residual_gate_stats(enc, ca, c_gate1, zero_floats=mp_e * (ff_ctx.fc1.rank + ff_ctx.fc2.rank),
                                               inplace=not keep_input)
    enc, e_stats, e_pool = residual_gate_stats(enc, ff_ctx(enc, ln=(e_stats, c_scale2, c_shift2, e_pool)), c_gate2,
                                               zero_floats=mp_e * attn.add_qkv_proj.rank, clamp_fp16=True)
    return enc, hidden, ((h_stats, h_pool), (e_stats, e_pool))
