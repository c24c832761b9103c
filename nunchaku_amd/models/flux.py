"""FLUX.1-shaped denoising transformer built on the SVDQuant hot path (stand-alone).

Structure and call pattern follow the reference's V2 model
(nunchaku/models/transformers/transformer_flux_v2.py:118-342,430-561,
 nunchaku/models/attention_processors/flux.py:71-108, nunchaku/models/normalization.py:85-165,
 nunchaku/models/attention.py:76-123): 19 joint + 38 single blocks, hidden 3072 = 24 x 128,
MLP x4; every 3072-wide projection is an ``SVDQW4A4Linear`` driven through
``fused_qkv_norm_rottary`` / ``fused_gelu_mlp`` / ``forward``.

``diffusers`` is not a dependency: the few non-quantised pieces it would provide (embedders,
AdaLayerNorm modulation) are restated here with plain torch ops.  The AdaLN modulation projections are
AWQ W4A16 GEMVs (``AWQW4A16Linear``) and attention runs on this library's kernel, as in the reference
(SURVEY.md section 8f items 1 and 3).  Used by bench.py with synthetic weights and by the GPU tests; a
reference checkpoint's SVDQ tensors load into the ``SVDQW4A4Linear`` members unchanged.  The fused path of the joint block
(the same computation as the Qwen-Image block's) is models/blocks.py; its reference-op path (``stats is None``) is here.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

from ..ops.attention import attention_packed, attention_packed_quantized, ip_attention, kv_valid_ranges, q_prescale
from ..ops.elementwise import ln_pool, modulated_diff, modulated_diff_scratch, residual_add_pair, residual_diff, residual_gate_stats
from ..ops.gemv import awq_gemv_w4a16_batched
from ..ops.fused import fused_gelu_mlp, fused_qkv_norm_rottary, fused_qkv_norm_rottary_pair, linear_pair, quantize_two
from ..utils import pad_tensor
from . import blocks
from .blocks import FeedForward as _FeedForward, _GELUProj, pad256 as _pad256  # noqa: F401  (the names this module has always had)
from .embeddings import flux_pos_embed, pack_rotemb
from .linear import AWQW4A16Linear, SVDQW4A4Linear


_FREQS: dict = {}


def timestep_embedding(t: torch.Tensor, dim: int = 256, max_period: float = 10000.0) -> torch.Tensor:
    """Sinusoidal embedding, (cos, sin) order, as diffusers' ``Timesteps(flip_sin_to_cos=True)``.  (The frequency table is a constant
    of (dim, period, device): built once -- three tiny launches less per call.)"""
    half = dim // 2
    key = (half, max_period, str(t.device))
    capturing = t.is_cuda and torch.cuda.is_current_stream_capturing()  # (a tensor made under capture lives in the graph's pool: not kept)
    freqs = None if capturing else _FREQS.get(key)
    if freqs is None:
        freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float32, device=t.device) / half)
        if not capturing:
            _FREQS[key] = freqs
    args = t.float()[:, None] * freqs[None]
    return torch.cat([args.cos(), args.sin()], dim=-1)


class _MLPEmbedder(nn.Module):
    def __init__(self, d_in, d, dtype, device):
        super().__init__()
        self.linear_1 = nn.Linear(d_in, d, dtype=dtype, device=device)
        self.linear_2 = nn.Linear(d, d, dtype=dtype, device=device)

    def forward(self, x):
        return self.linear_2(F.silu(self.linear_1(x)))


class _TimeTextEmbed(nn.Module):
    """diffusers' CombinedTimestep(Guidance)TextProjEmbeddings: ``timestep_embedder`` / ``guidance_embedder`` / ``text_embedder``,
    each ``linear_1 -> SiLU -> linear_2``."""

    def __init__(self, dim, pooled_dim, guidance, dtype, device):
        super().__init__()
        self.timestep_embedder = _MLPEmbedder(256, dim, dtype, device)
        self.guidance_embedder = _MLPEmbedder(256, dim, dtype, device) if guidance else None
        self.text_embedder = _MLPEmbedder(pooled_dim, dim, dtype, device)


class FluxAttentionAMD(nn.Module):
    """Joint (img + txt) or single-stream attention with fused QKV/RMSNorm/RoPE projections."""

    def __init__(self, dim, heads, joint: bool, kw):
        super().__init__()
        self.heads, self.head_dim = heads, dim // heads
        self.to_qkv = SVDQW4A4Linear(dim, 3 * dim, **kw)
        self.norm_q = nn.RMSNorm(self.head_dim, eps=1e-6, dtype=kw["torch_dtype"], device=kw["device"])
        self.norm_k = nn.RMSNorm(self.head_dim, eps=1e-6, dtype=kw["torch_dtype"], device=kw["device"])
        # diffusers' FluxAttention keeps `to_out = [Linear, Dropout]` in joint blocks (checkpoint key `attn.to_out.0`); the
        # single blocks' output projection is the V2 key `attn.to_out` (transformer_flux_v2.py:564-625)
        self.to_out = nn.ModuleList([SVDQW4A4Linear(dim, dim, **kw), nn.Identity()]) if joint else SVDQW4A4Linear(dim, dim, **kw)
        self.joint = joint
        self.added_kv_proj_dim = dim if joint else None  # the attribute the reference's processors test (flux.py:84,177)
        if joint:
            self.add_qkv_proj = SVDQW4A4Linear(dim, 3 * dim, **kw)
            self.norm_added_q = nn.RMSNorm(self.head_dim, eps=1e-6, dtype=kw["torch_dtype"], device=kw["device"])
            self.norm_added_k = nn.RMSNorm(self.head_dim, eps=1e-6, dtype=kw["torch_dtype"], device=kw["device"])
            self.to_add_out = SVDQW4A4Linear(dim, dim, **kw)

    # "svdq": this library's attention kernel on the packed QKV (+ V^T side output of the QKV GEMM);
    # "sdpa": torch's scaled_dot_product_attention (the reference's "flashattn2" processor role,
    # models/attention_processors/flux.py:24-59).  "svdq" needs B == 1, head_dim 128, tokens % 128 == 0.
    attention_impl = "svdq"
    # True: the text and image stream's projections of a joint block share one GEMM launch each (svdq_gemm_args.wgt2)
    grouped = True  # plain class attribute (set False for A/B runs); nothing is read from the environment
    # True: the attention epilogue emits the output projection's quantised activation (svdq_attention_args.qact)
    fused_out_quant = True
    # True: the engine pads both token streams to 256 rows so that every token count runs the fused path (False: A/B -- token counts that
    # are not a multiple of 128 then take torch's SDPA)
    padded_tokens = True

    @property
    def out_proj(self) -> SVDQW4A4Linear:
        return self.to_out[0] if self.joint else self.to_out

    def _use_svdq(self, B, tokens):
        return self.attention_impl == "svdq" and B == 1 and self.head_dim == 128 and tokens % 128 == 0

    def forward(self, hidden, encoder_hidden=None, rotary=None, ln=None, ln_ctx=None, quantized=None, kv_valid=None):
        """``ln`` / ``ln_ctx`` = (stats, scale, shift): the inputs are the UN-normalised streams and the
        AdaLayerNormZero front end runs inside the QKV projections' quantiser.  ``kv_valid``: the real key rows when the
        streams are padded to 256 rows (the engine pads every token count onto this path; ``ops.attention.kv_valid_ranges``)."""
        B, hd = hidden.shape[0], self.heads * self.head_dim
        t_txt = encoder_hidden.shape[1] if self.joint else 0
        tokens = t_txt + hidden.shape[1]
        svdq = self._use_svdq(B, tokens)
        if self.joint and svdq and self.grouped and len(rotary) > 2:  # every launch serves both streams (svdq: B == 1)
            out = blocks.joint_attention(self, hidden, encoder_hidden, rotary[2], ln, ln_ctx, kv_valid, quantized=self.fused_out_quant)
            if out is not None:
                return out
        qs = q_prescale(self.head_dim) if svdq else 0.0  # the QKV GEMM emits Q times scale * log2(e): the attention kernel's fast geometry
        qkv = torch.empty(B, tokens, 3 * hd, dtype=hidden.dtype, device=hidden.device)
        vt = torch.empty(hd, tokens, dtype=hidden.dtype, device=hidden.device) if svdq else None
        if self.joint:
            # both projections write straight into one [txt; img] buffer (B == 1): no torch.cat round trip
            grouped = False
            if self.grouped and B == 1 and len(rotary) > 2 and not svdq:  # torch's attention on the grouped projections (svdq: declined above)
                grouped = fused_qkv_norm_rottary_pair(encoder_hidden, self.add_qkv_proj, self.norm_added_q, self.norm_added_k,
                                                      hidden, self.to_qkv, self.norm_q, self.norm_k, rotary[2], qkv[0],
                                                      out_vt=vt, ln_a=ln_ctx, ln_b=ln, q_scale=qs)
            if not grouped:  # the two projections cannot share a launch: one each
                fused_qkv_norm_rottary(hidden, self.to_qkv, self.norm_q, self.norm_k, rotary[0], output=qkv[0, t_txt:],
                                       out_vt=vt[:, t_txt:] if svdq else None, ln=ln, q_scale=qs)
                fused_qkv_norm_rottary(encoder_hidden, self.add_qkv_proj, self.norm_added_q, self.norm_added_k, rotary[1],
                                       output=qkv[0, :t_txt], out_vt=vt[:, :t_txt] if svdq else None, ln=ln_ctx, q_scale=qs)
            if svdq and self.grouped:
                return blocks.joint_attention_out(self, qkv[0], vt, t_txt, ln_pool(ln_ctx), kv_valid, quantized=self.fused_out_quant)
        else:
            fused_qkv_norm_rottary(hidden, self.to_qkv, self.norm_q, self.norm_k, rotary, output=qkv.view(B * tokens, -1),
                                   out_vt=vt, ln=ln, quantized=quantized, q_scale=qs)
            if svdq and self.fused_out_quant:
                qres = attention_packed_quantized(qkv[0], vt, self.heads, self.out_proj, pool=ln_pool(ln), q_prescaled=True, kv_valid=kv_valid)
                if qres is not None:  # the 16-bit attention output never exists: straight into the output projection
                    return self.out_proj.forward_quant(*qres).view(B, tokens, -1)
        pool = None
        if svdq:  # the same launch clears the low-rank accumulators of the output projections' quantisers
            zf = _pad256(hidden.shape[1]) * self.out_proj.rank + (_pad256(t_txt) * self.to_add_out.rank if self.joint else 0)
            o, pool = attention_packed(qkv[0], vt, self.heads, zero_floats=zf, q_prescaled=True, kv_valid=kv_valid)
            o = o.unsqueeze(0)
        else:
            q, k, v = qkv.chunk(3, dim=-1)
            shp = (B, -1, self.heads, self.head_dim)
            o = F.scaled_dot_product_attention(q.view(shp).transpose(1, 2), k.view(shp).transpose(1, 2),
                                               v.view(shp).transpose(1, 2), dropout_p=0.0, is_causal=False)
            o = o.transpose(1, 2).reshape(B, -1, hd)
        if self.joint:
            if self.grouped and B == 1:
                ca, a = linear_pair(o[:, :t_txt], self.to_add_out, o[:, t_txt:], self.out_proj, pool=pool)
                return a, ca
            return self.out_proj(o[:, t_txt:], pool=pool), self.to_add_out(o[:, :t_txt], pool=pool)
        return self.out_proj(o, pool=pool)


class _AdaLNZero(nn.Module):
    """Parameter holder with the reference's / diffusers' module name: ``norm1.linear`` = the AdaLayerNormZero modulation
    projection, an AWQ W4A16 GEMV (normalization.py:85-98, linear.py:277-414).  The LayerNorm itself has no parameters and
    runs inside the quantiser (fused path) or as a torch op (block forward)."""

    def __init__(self, dim, chunks, dt, dev):
        super().__init__()
        self.linear = AWQW4A16Linear(dim, chunks * dim, torch_dtype=dt, device=dev)
        self.linear.out_chunks = chunks  # the GEMV writes the `chunks` [dim] vectors contiguously


class FluxJointBlockAMD(nn.Module):
    """reference: NunchakuFluxTransformerBlock (transformer_flux_v2.py:143-257); same sub-module names, so a V2 checkpoint's
    keys (``transformer_blocks.N.norm1.linear.qweight``, ``...attn.to_out.0.proj_up``, ``...ff.net.0.proj.wscales``) load as they are."""

    def __init__(self, dim, heads, kw):
        super().__init__()
        dt, dev = kw["torch_dtype"], kw["device"]
        self.norm1 = _AdaLNZero(dim, 6, dt, dev)
        self.norm1_context = _AdaLNZero(dim, 6, dt, dev)
        self.attn = FluxAttentionAMD(dim, heads, True, kw)
        self.ff = _FeedForward(dim, kw)
        self.ff_context = _FeedForward(dim, kw)
        self.dim = dim

    @property
    def mod(self) -> AWQW4A16Linear:
        return self.norm1.linear

    @property
    def mod_context(self) -> AWQW4A16Linear:
        return self.norm1_context.linear

    @staticmethod
    def _ln_mod(x, scale, shift):
        # NunchakuAdaLayerNormZero with scale_shift = 0 (normalization.py:85-98): the checkpoint's modulation bias
        # already carries the +1 of the scale
        return F.layer_norm(x, (x.shape[-1],), eps=1e-6) * scale[:, None] + shift[:, None]

    def forward(self, hidden, encoder_hidden, temb_act, rotary, stats=None, mods=None, kv_valid=None, keep_input=False):
        """``mods`` = (mod, mod_context) outputs computed ahead of the block (one batched GEMV launch per step).
        ``keep_input``: the fused path leaves ``hidden`` / ``encoder_hidden`` as they are (its first residual pass writes new tensors
        instead of updating the streams in place; same launches) -- First-Block Cache needs a block's input after the block.
        ``stats`` = (image-stream, text-stream) LayerNorm statistics of the inputs: the fused path -- LayerNorm and
        modulation inside the quantisers, gated residual + next statistics in one element-wise pass (B == 1).
        Returns (encoder_hidden, hidden, stats)."""
        # normalization.py:85-98 -- emb.view(B, -1, 6).permute(2, 0, 1): interleaved chunks
        if stats is None:
            m = self.mod(temb_act).view(temb_act.shape[0], 6, -1).permute(1, 0, 2)
            c = self.mod_context(temb_act).view(temb_act.shape[0], 6, -1).permute(1, 0, 2)
            shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = m
            c_shift_msa, c_scale_msa, c_gate_msa, c_shift_mlp, c_scale_mlp, c_gate_mlp = c
            n_h = self._ln_mod(hidden, scale_msa, shift_msa)
            n_e = self._ln_mod(encoder_hidden, c_scale_msa, c_shift_msa)
            a, ca = self.attn(n_h, n_e, rotary, kv_valid=kv_valid)
            hidden = hidden + gate_msa[:, None] * a  # transformer_flux_v2.py:230-251, op for op
            n_h = self._ln_mod(hidden, scale_mlp, shift_mlp)
            hidden = hidden + gate_mlp[:, None] * self.ff(n_h)
            encoder_hidden = encoder_hidden + c_gate_msa[:, None] * ca
            n_e = self._ln_mod(encoder_hidden, c_scale_mlp, c_shift_mlp)
            encoder_hidden = encoder_hidden + c_gate_mlp[:, None] * self.ff_context(n_e)
            if encoder_hidden.dtype == torch.float16:  # transformer_flux_v2.py: the fp16 joint block clips its text stream
                encoder_hidden = encoder_hidden.clip(-65504, 65504)
            return encoder_hidden, hidden, None
        m_out, c_out = mods if mods is not None else (self.mod(temb_act), self.mod_context(temb_act))
        # the reference clips the text stream only at the end of an fp16 joint block (transformer_flux_v2.py)
        return blocks.dual_stream_block(
            lambda h, e, ln, ln_ctx: self.attn(h, e, rotary, ln=ln, ln_ctx=ln_ctx, kv_valid=kv_valid), self.attn, self.ff, self.ff_context,
            hidden, encoder_hidden, stats, m_out, c_out, clamp_img=False, keep_input=keep_input, grouped=self.attn.grouped)


class FluxSingleBlockAMD(nn.Module):
    """reference: NunchakuFluxSingleTransformerBlock (transformer_flux_v2.py:260-342): ``norm.linear``, ``attn.to_qkv``,
    ``attn.to_out``, ``mlp_fc1``, ``mlp_fc2``."""

    def __init__(self, dim, heads, kw):
        super().__init__()
        dt, dev = kw["torch_dtype"], kw["device"]
        self.norm = _AdaLNZero(dim, 3, dt, dev)  # AdaLayerNormZeroSingle.linear (normalization.py:155-165)
        self.mlp_fc1 = SVDQW4A4Linear(dim, 4 * dim, **kw)
        self.mlp_fc2 = SVDQW4A4Linear(4 * dim, dim, **{**kw, "act_unsigned": True})
        self.attn = FluxAttentionAMD(dim, heads, False, kw)

    @property
    def mod(self) -> AWQW4A16Linear:
        return self.norm.linear

    def forward(self, hidden, temb_act, rotary, stats=None, mods=None, kv_valid=None, keep_input=False):
        """``keep_input``: the fused path writes its result to a new tensor instead of updating ``hidden`` in place (same launch)."""
        if stats is None:
            shift, scale, gate = self.mod(temb_act).view(temb_act.shape[0], 3, -1).permute(1, 0, 2)
            n = F.layer_norm(hidden, (hidden.shape[-1],), eps=1e-6) * scale[:, None] + shift[:, None]
            mlp = fused_gelu_mlp(n, self.mlp_fc1, self.mlp_fc2)
            att = self.attn(n, rotary=rotary, kv_valid=kv_valid)
            out = hidden + gate[:, None] * (att + mlp)  # transformer_flux_v2.py:332-335
            if out.dtype == torch.float16:
                out = out.clip(-65504, 65504)
            return out, None
        shift, scale, gate = (mods if mods is not None else self.mod(temb_act)).view(3, -1)
        st, pool = stats
        ln = (st, scale, shift, pool)  # one LayerNorm + modulation, consumed by both projections' quantisers
        both = quantize_two(hidden, self.mlp_fc1, self.attn.to_qkv, ln=ln) if FluxAttentionAMD.grouped else None
        q_mlp, q_qkv = both if both is not None else (None, None)  # one quantiser launch for the two projections
        mlp = fused_gelu_mlp(hidden, self.mlp_fc1, self.mlp_fc2, ln=ln, quantized=q_mlp)
        att = self.attn(hidden, rotary=rotary, ln=ln, quantized=q_qkv, kv_valid=kv_valid)
        # hidden + gate * (att + mlp), the next block's statistics and its three low-rank accumulators, one pass
        hidden, st, pool = residual_gate_stats(hidden, att, gate, b=mlp, zero_floats=_pad256(hidden.shape[1]) * (
            self.mlp_fc1.rank + self.mlp_fc2.rank + self.attn.to_qkv.rank + self.attn.out_proj.rank), clamp_fp16=True, inplace=not keep_input)
        return hidden, (st, pool)


def _ids_versions(*ids):
    """version counters of the position-id tensors, or None when one of them does not track a version (inference tensors raise on ._version)"""
    try:
        return tuple(None if t is None else t._version for t in ids) if not any(t is not None and t.is_inference() for t in ids) else None
    except RuntimeError:
        return None


class FluxEngineMixin:
    """Everything of the FLUX.1 transformer that is not construction: the denoising-step forward over the module tree
    ``x_embedder / context_embedder / time_text_embed / transformer_blocks / single_transformer_blocks / norm_out / proj_out``
    (diffusers' names), the runtime-LoRA entry points and the synthetic initialiser.  Shared by the stand-alone
    :class:`FluxTransformerAMD` and -- when diffusers is importable -- the ``diffusers.FluxTransformer2DModel`` subclass of
    nunchaku_amd/models/transformer_flux.py, whose sub-modules are these same classes."""

    # True: AdaLayerNormZero runs inside the quantisers and the gated residuals are one fused pass each
    # (svdq_quantize_args.ln_stats, svdq_residual_gate_stats); False: the reference's torch-op sequence.
    fused_norm = True
    # True: all modulation GEMVs of a step in one batched launch before the first block
    batched_mods = True

    def _build_engine(self, num_layers=19, num_single_layers=38, dim=3072, heads=24, in_channels=64,
                      joint_attention_dim=4096, pooled_projection_dim=768, rank=32, guidance_embeds=True,
                      axes_dims_rope=(16, 56, 56), torch_dtype=torch.bfloat16, device="cuda"):
        """Create (or replace) the module tree on ``device``; parameters are uninitialised (load a checkpoint next)."""
        kw = dict(rank=rank, torch_dtype=torch_dtype, device=device)
        self.dim, self.axes = dim, tuple(axes_dims_rope)
        self.x_embedder = nn.Linear(in_channels, dim, dtype=torch_dtype, device=device)
        self.context_embedder = nn.Linear(joint_attention_dim, dim, dtype=torch_dtype, device=device)
        # module names = diffusers' FluxTransformer2DModel / the reference's V2 model: V2 checkpoints load key for key
        self.time_text_embed = _TimeTextEmbed(dim, pooled_projection_dim, guidance_embeds, torch_dtype, device)
        self.transformer_blocks = nn.ModuleList([FluxJointBlockAMD(dim, heads, kw) for _ in range(num_layers)])
        self.single_transformer_blocks = nn.ModuleList([FluxSingleBlockAMD(dim, heads, kw) for _ in range(num_single_layers)])
        self.norm_out = blocks.AdaLNContinuous(dim, torch_dtype, device)
        self.proj_out = nn.Linear(dim, in_channels, dtype=torch_dtype, device=device)
        self.dtype_ = torch_dtype
        self._dense_lora: dict = {}  # LoRA deltas merged into 16-bit parameters: name -> (parameter, copy of its original data, fp32 delta at strength 1)

    # short names used throughout this package (and by its tests / tools)
    @property
    def blocks(self):
        return self.transformer_blocks

    @property
    def single_blocks(self):
        return self.single_transformer_blocks

    @property
    def time_embed(self):
        return self.time_text_embed.timestep_embedder

    @property
    def guidance_embed(self):
        return self.time_text_embed.guidance_embedder

    @property
    def text_embed(self):
        return self.time_text_embed.text_embedder

    @property
    def norm_out_mod(self):
        return self.norm_out.linear

    def svdq_layers(self):
        return [m for m in self.modules() if isinstance(m, SVDQW4A4Linear)]

    def set_attention_impl(self, impl: str, attn_func=None):
        """reference: NunchakuFluxTransformer2dModel.set_attention_impl (transformer_flux.py:648-667).  ``"nunchaku-fp16"``:
        the attention kernel of this library fed by the QKV epilogue (its role on MI355X; bf16 and fp16);
        ``"flashattn2"``: ``torch.nn.functional.scaled_dot_product_attention``."""
        table = {"nunchaku-fp16": "svdq", "svdq": "svdq", "flashattn2": "sdpa", "sdpa": "sdpa"}
        if impl == "custom" or attn_func is not None:
            raise NotImplementedError("set_attention_impl: custom attention functions are not supported")
        if impl not in table:
            raise ValueError(f"set_attention_impl: unknown implementation {impl!r}")
        for m in self.modules():
            if isinstance(m, FluxAttentionAMD):
                m.attention_impl = table[impl]

    # runtime LoRA (reference: NunchakuFluxTransformer2dModel.update_lora_params / set_lora_strength,
    # transformer_flux.py:783-855): per-layer factors in logical layout widen the low-rank branch of that layer
    @torch.no_grad()
    def update_lora_params(self, lora, strength: float = 1.0):
        """``lora``: a diffusers / PEFT LoRA -- the path of a ``.safetensors`` file (``str`` / ``os.PathLike``) or its state dict
        (``<module>.lora_A.weight`` / ``.lora_B.weight`` [/ ``.alpha``] keys, ``transformer.`` prefix optional: converted by
        ``nunchaku_amd.lora.flux.to_engine_lora``) -- or, as before, ``{engine module name: (down [r, in], up [out, r])}``
        (e.g. ``"transformer_blocks.0.attn.to_qkv"``; a 1-D tensor under ``"<module name>.bias"`` is a bias delta).  Replaces a LoRA attached earlier.
        ``SVDQW4A4Linear`` and ``AWQW4A16Linear`` targets get a low-rank branch (``set_lora``); ``nn.Linear`` targets (embedders, ``norm_out.linear``,
        ``proj_out``) are merged, ``W += strength * up @ down``, with the original kept for :meth:`reset_lora` / :meth:`set_lora_strength`.
        Attaching, rescaling or removing a LoRA changes tensor shapes, kernel arguments (the strengths) or launches: a captured step
        (``graph.CapturedStep``) has to be captured again afterwards, as with ``SVDQW4A4Linear.set_lora``.
        A nunchaku-format LoRA (``lora_down`` / ``lora_up`` / ``qweight`` keys) raises ``NotImplementedError``; keys that fit nothing ``KeyError``."""
        import os

        from ..lora import flux as lora_flux

        if isinstance(lora, (str, os.PathLike)):
            lora = lora_flux.load_state_dict(lora)
        if lora_flux.is_nunchaku_format(lora) or lora_flux.is_peft_format(lora):
            lora = lora_flux.to_engine_lora(lora, self)
        mods = dict(self.named_modules())
        bad = [n for n, v in lora.items() if not (isinstance(mods.get(n), (SVDQW4A4Linear, AWQW4A16Linear, nn.Linear)) and isinstance(v, (tuple, list)))
               and not (n.endswith(".bias") and getattr(mods.get(n[:-5]), "bias", None) is not None and torch.is_tensor(v))]
        if bad:
            raise KeyError(f"update_lora_params: {bad} name no SVDQW4A4Linear, AWQW4A16Linear or nn.Linear (or '<module>.bias') of this model, "
                           "and are no diffusers / PEFT LoRA keys (<module>.lora_A.weight / <module>.lora_B.weight)")
        self.reset_lora()
        for name, v in lora.items():
            if name not in mods:  # "<module>.bias": original kept, delta merged below
                layer = mods[name[:-5]]
                if isinstance(layer, SVDQW4A4Linear):
                    layer._ensure_layout()  # the kernel layout of a bias is the natural order
                self._dense_lora[name] = (layer.bias, layer.bias.data.clone(), v.reshape(-1).to(layer.bias.device, torch.float32))
            elif isinstance(mods[name], nn.Linear):
                w = mods[name].weight
                down, up = v
                if tuple(up.shape) != (w.shape[0], down.shape[0]) or down.shape[1] != w.shape[1]:
                    raise ValueError(f"update_lora_params: {name}: expected down [r, {w.shape[1]}] and up [{w.shape[0]}, r]")
                self._dense_lora[name] = (w, w.data.clone(), up.to(w.device, torch.float32) @ down.to(w.device, torch.float32))
            else:
                mods[name].set_lora(v[0], v[1], strength)
        self._merge_dense_lora(strength)

    def _merge_dense_lora(self, strength: float):
        """16-bit parameter = round16(original + strength * delta), the sum in fp32"""
        for param, orig, delta in self._dense_lora.values():
            param.data.copy_((orig.float() + float(strength) * delta).to(orig.dtype))  # in place: whoever holds the storage sees the new weights

    def lora_layers(self):
        return [m for m in self.modules() if isinstance(m, (SVDQW4A4Linear, AWQW4A16Linear))]

    @torch.no_grad()
    def set_lora_strength(self, strength: float):
        for m in self.lora_layers():
            if (m._base_lowrank if isinstance(m, SVDQW4A4Linear) else m._lora) is not None:
                m.set_lora_strength(strength)
        self._merge_dense_lora(strength)

    @torch.no_grad()
    def reset_lora(self):
        for m in self.lora_layers():
            m.reset_lora()
        for param, orig, _ in self._dense_lora.values():
            param.data.copy_(orig)
        self._dense_lora.clear()

    @torch.no_grad()
    def init_synthetic_(self, seed: int = 0, repack: bool = True, codes: str = "uniform"):
        """Random-init weights of FLUX shape (models/blocks.py ``init_synthetic_``), repacked like a loaded checkpoint."""
        return blocks.init_synthetic_(self, seed, codes, repack=repack, awq_scale_one=True)

    def engine_forward(self, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids,
                       guidance=None, controlnet_block_samples=None, controlnet_single_block_samples=None, controlnet_blocks_repeat=False,
                       *, ip_hidden_states=None, id_embeddings=None, id_weight=1.0):
        """hidden_states [1, T_img, 64]; encoder_hidden_states [1, T_txt, 4096]; pooled [1, 768];
        timestep/guidance [1]; img_ids [T_img, 3]; txt_ids [T_txt, 3]  ->  [1, T_img, 64]
        (transformer_flux_v2.py:430-561; batch 1 -- the fused QKV epilogue takes one rotary table).
        ``controlnet_block_samples`` / ``controlnet_single_block_samples``: lists of ``[1, T_img, dim]`` residuals added to the image
        stream behind the joint / single blocks with diffusers' indexing (``FluxTransformer2DModel.forward``: sample
        ``i // ceil(blocks / samples)``, or ``i % samples`` with ``controlnet_blocks_repeat``).
        ``ip_hidden_states``: the image embeddings of an attached IP-Adapter (``models/ip_adapter.py``) -- a tensor whose last axis is the
        adapter's ``cross_dim`` and whose other axes are all image-prompt tokens, or the pipeline's list (element 0); None: the stored
        ``image_embeds``.  Ignored without an adapter; an adapter without any embeddings raises ``ValueError``.
        ``id_embeddings`` / ``id_weight``: PuLID (``models/pulid.py``; needs ``attach_pulid``) -- the identity embeddings ``[1, N, kv_dim]``
        (N <= 32 on the fused arm) and the strength, a Python float: behind every second joint and every fourth single block the image
        stream gets ``id_weight * pulid_ca[k](id_embeddings, hidden)``.  Batch 1 only; refused with a cache active or an offloaded model.
        The step is its stages run back to back (``_prologue``, ``_run_joint``, ``_join``, ``_run_single``, ``_tail``);
        :meth:`engine_forward_cached` is the same stages with the First-Block-Cache decision in between."""
        if id_embeddings is not None:
            self._pulid_check(hidden_states)
        if hidden_states.shape[0] > 1:
            # The fused QKV epilogue takes ONE rotary table and the operand buffers of a launch belong to one sample
            # (reference: rotary_emb.shape[0] * shape[1] == M assert, launch_impl.cuh:353): a batch
            # is a loop over samples here -- the data-parallel unit of this library is the replica, not the batch axis.
            def per(t, i):
                return t[i:i + 1] if t is not None and t.dim() > 0 and t.shape[0] == hidden_states.shape[0] else t
            def per_list(ts, i):
                return None if ts is None else [per(t, i) for t in ts]
            def per_ip(i):  # the embeddings of sample i when they carry a batch axis of this batch's size ([B, tokens, cross_dim] or more axes)
                t = ip_hidden_states[0] if isinstance(ip_hidden_states, (list, tuple)) and len(ip_hidden_states) else ip_hidden_states
                return t[i:i + 1] if torch.is_tensor(t) and t.dim() >= 3 and t.shape[0] == hidden_states.shape[0] else t
            return torch.cat([self.engine_forward(hidden_states[i:i + 1], encoder_hidden_states[i:i + 1], pooled_projections[i:i + 1],
                                           per(timestep, i), img_ids, txt_ids, per(guidance, i), per_list(controlnet_block_samples, i),
                                           per_list(controlnet_single_block_samples, i), controlnet_blocks_repeat,
                                           ip_hidden_states=per_ip(i))
                              for i in range(hidden_states.shape[0])], dim=0)
        st = self._prologue(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance,
                            controlnet_block_samples, controlnet_single_block_samples, controlnet_blocks_repeat, ip_hidden_states=ip_hidden_states,
                            id_embeddings=id_embeddings, id_weight=id_weight)
        # every modulation projection depends on the timestep embedding only: one batched GEMV launch for the whole step
        self._launch_mods(st, range(len(self.blocks)), range(len(self.single_blocks)))
        self._run_joint(st, 0, len(self.blocks))
        self._join(st)
        self._run_single(st, 0, len(self.single_blocks))
        return self._tail(st)

    def _prologue(self, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None,
                  controlnet_block_samples=None, controlnet_single_block_samples=None, controlnet_blocks_repeat=False, *,
                  ip_hidden_states=None, id_embeddings=None, id_weight=1.0) -> "_Step":
        """Embedders, rotary tables, padding of the two streams and their first LayerNorm statistics; with an IP-Adapter attached, the
        image-prompt K / V of every joint block (projected once per embeddings tensor: ``IPAdapter.kv``)."""
        dt = self.dtype_
        adapter = getattr(self, "ip_adapter", None)
        ip_kv = None if adapter is None else adapter.kv(adapter.resolve(ip_hidden_states))  # (raises before anything is launched)
        hidden = self.x_embedder(hidden_states)
        # diffusers casts timestep / guidance to the model dtype BEFORE the x1000 (transformer_flux.py: timestep.to(dtype) * 1000)
        temb = self.time_embed(timestep_embedding(timestep.to(dt) * 1000).to(dt))
        if self.guidance_embed is not None:
            temb = temb + self.guidance_embed(timestep_embedding(guidance.to(dt) * 1000).to(dt))
        temb = temb + self.text_embed(pooled_projections)
        temb_act = F.silu(temb)
        enc = self.context_embedder(encoder_hidden_states)

        t_txt, t_img = enc.shape[1], hidden.shape[1]
        attn0 = (self.blocks[0] if len(self.blocks) else self.single_blocks[0]).attn
        pad_streams = FluxAttentionAMD.padded_tokens and attn0.attention_impl == "svdq" and attn0.head_dim == 128
        # the rotary tables depend on the position ids only: a denoise loop passes the same two tensor OBJECTS every step -- built once and kept
        # (one entry; the cache holds the id tensors themselves, so "the same object, unmodified" cannot be a recycled address).  Not cached:
        #  * ids whose version counter cannot be read (tensors created under torch.inference_mode() do not track one): "unmodified" is unknowable;
        #  * while the stream is capturing: the tables are computed INSIDE the graph (its pool owns them and ids passed as static graph inputs
        #    keep their meaning on replay); a graph must never bake in pointers to tables that only this one-entry cache keeps alive -- a later
        #    eager call with other ids would free them under the graph (same hazard as _Workspace.captured, _C.release_workspaces).
        vers = _ids_versions(txt_ids, img_ids)
        use_cache = vers is not None and not (hidden.is_cuda and torch.cuda.is_current_stream_capturing())
        key = (vers, pad_streams)
        cached = getattr(self, "_rot_cache", None) if use_cache else None
        if cached is not None and cached[0] is txt_ids and cached[1] is img_ids and cached[2] == key:
            rot_txt, rot_img, rot_all, p_txt, p_img = cached[3]
        else:
            rot = flux_pos_embed(torch.cat([txt_ids, img_ids], dim=0), self.axes)  # [1, T, 64, 1, 2]
            rot_t, rot_i = pad_tensor(rot[:, :t_txt], 256, 1), pad_tensor(rot[:, t_txt:], 256, 1)
            rot_txt, rot_img = pack_rotemb(rot_t), pack_rotemb(rot_i)
            p_txt, p_img = rot_t.shape[1], rot_i.shape[1]
            # joint table: every stream on a 256-row boundary when the streams are padded (below), the plain concatenation otherwise
            rot_all = pack_rotemb(torch.cat([rot_t, rot_i], dim=1)) if pad_streams and kv_valid_ranges(t_txt, t_img) is not None \
                else pack_rotemb(pad_tensor(rot, 256, 1))
            if use_cache:
                self._rot_cache = (txt_ids, img_ids, key, (rot_txt, rot_img, rot_all, p_txt, p_img))
        # EVERY token count runs the hot path (the reference pads any M to 256 rows, Linear.cpp:445-446, and masks the padded K rows of its
        # attention, epilogues.cuh:427-550): both streams are padded to 256 rows with zero tokens right behind the embedders -- the joint
        # sequence is [text | pad | image | pad], every stream starts on a 256-row boundary as the grouped launches need -- every launch of
        # the step sees the shapes the parity suite and the bench exercise, the attention kernel masks the padded keys (kv_valid), and the
        # real image rows are sliced out at the end.  A padded row is a token nobody attends to: it stays finite and touches no real row.
        kv_valid = kv_valid_ranges(t_txt, t_img) if pad_streams else None
        if kv_valid is not None:
            enc, hidden = F.pad(enc, (0, 0, 0, p_txt - t_txt)), F.pad(hidden, (0, 0, 0, p_img - t_img))
        else:
            p_txt = t_txt

        st = _Step()
        st.hidden, st.enc, st.temb_act, st.rot, st.kv_valid = hidden, enc, temb_act, (rot_img, rot_txt, rot_all), kv_valid
        st.t_txt, st.t_img, st.p_txt, st.joined, st.mods = t_txt, t_img, p_txt, False, {}
        st.cn_joint, st.cn_single, st.cn_repeat = controlnet_block_samples, controlnet_single_block_samples, controlnet_blocks_repeat
        st.fused = self.fused_norm and hidden.shape[0] == 1
        st.ip = None if adapter is None else (ip_kv, adapter.ip_adapter_scale)
        st.pulid = None if id_embeddings is None else (self.pulid_ca, id_embeddings, float(id_weight), self.pulid_fused and st.fused)
        st.stats = ((residual_gate_stats(hidden)[1], None), (residual_gate_stats(enc)[1], None)) if st.fused else None
        return st

    def _launch_mods(self, st: "_Step", joint, single) -> None:
        """The modulation projections of the joint blocks ``joint`` and the single blocks ``single`` (index ranges) in one batched GEMV
        launch; a block whose projections were not launched here runs its own."""
        if not (st.fused and self.batched_mods):
            return
        lins = [m for i in joint for m in (self.blocks[i].mod, self.blocks[i].mod_context)] + [self.single_blocks[i].mod for i in single]
        if not lins:
            return
        outs = awq_gemv_w4a16_batched(st.temb_act, lins)
        for k, i in enumerate(joint):
            st.mods["j", i] = (outs[2 * k], outs[2 * k + 1])
        for k, i in enumerate(single):
            st.mods["s", i] = outs[2 * len(joint) + k]

    def _run_joint(self, st: "_Step", lo: int, hi: int, keep_input: bool = False) -> None:
        """Joint blocks ``lo .. hi - 1``.  ``keep_input``: block ``lo`` leaves its two input tensors as they are (the fused path updates the
        streams in place otherwise)."""
        nj = len(self.blocks)
        for i in range(lo, hi):
            st.enc, st.hidden, st.stats = self.blocks[i](st.hidden, st.enc, st.temb_act, st.rot, st.stats, mods=st.mods.get(("j", i)),
                                                         kv_valid=st.kv_valid, keep_input=keep_input and i == lo)
            ip_q = self._ip_query(st, i) if st.ip is not None else None  # of the block's output, BEFORE the ControlNet residual (the reference's order)
            if st.cn_joint is not None:
                st.hidden, h_stats = blocks.add_control(st.hidden, st.cn_joint, i, nj, st.cn_repeat, want_stats=st.fused)
                if st.fused:
                    st.stats = ((h_stats, st.stats[0][1]), st.stats[1])
            if st.pulid is not None and i % 2 == 0:
                self._pulid_add(st, i // 2)
            if st.ip is not None:
                self._ip_add(st, i, ip_q)

    def _ip_fused(self, st: "_Step", attn) -> bool:
        """the adapter's step runs on this library's kernels (else: the reference's torch-op sequence)"""
        return st.fused and attn.attention_impl == "svdq" and attn.head_dim == 128

    def _ip_query(self, st: "_Step", i: int) -> torch.Tensor:
        """The IP-Adapter query of joint block ``i`` (reference: FluxModel.cpp ``get_q_heads``): NOT the Q its attention used but the
        block's OUTPUT image stream through this block's ``norm1`` modulation (shift_msa / scale_msa), ``to_qkv``, ``norm_q`` and RoPE
        with the image table -- a second QKV projection per joint block, kept because it is the reference's arithmetic.  Returns the
        packed ``[tokens, 3 * dim]`` projection output; its Q third is the query (prescaled by ``q_prescale`` on the fused arm)."""
        blk = self.blocks[i]
        attn = blk.attn
        hidden = st.hidden
        if self._ip_fused(st, attn):
            mods = st.mods.get(("j", i))
            shift_msa, scale_msa = (mods[0] if mods is not None else blk.mod(st.temb_act)).view(6, -1)[:2]
            # LayerNorm + modulation inside the quantiser, from the statistics that came out of the block's last residual pass.  No
            # ZeroPool in this tuple: the pools in st.stats belong to the NEXT block's launches; this quantiser clears its own accumulator.
            ln = (st.stats[0][0], scale_msa, shift_msa)
            return fused_qkv_norm_rottary(hidden, attn.to_qkv, attn.norm_q, attn.norm_k, st.rot[0], ln=ln,
                                          q_scale=q_prescale(attn.head_dim))[0]
        m = blk.mod(st.temb_act).view(st.temb_act.shape[0], 6, -1).permute(1, 0, 2)
        return fused_qkv_norm_rottary(blk._ln_mod(hidden, m[1], m[0]), attn.to_qkv, attn.norm_q, attn.norm_k, st.rot[0])[0]

    def _ip_add(self, st: "_Step", i: int, qkv: torch.Tensor) -> None:
        """``hidden += ip_adapter_scale * SDPA(ip_query, k_img, v_img)`` behind joint block ``i`` (reference: ip_adapter/utils.py:361-372).
        Fused arm: one ``svdq_ip_attention`` launch on the packed buffer (the strength multiplies in fp32 inside it, as torch's
        ``float * tensor``), then ONE ``svdq_residual_gate_stats`` pass that adds it and delivers the statistics the next block's
        quantisers need -- the image stream must not change behind the pass that produced its statistics.  Padded image rows take part
        like any row: tokens nobody reads."""
        kv, scale = st.ip
        k_img, v_img = kv[i]
        attn = self.blocks[i].attn
        if self._ip_fused(st, attn):
            o = ip_attention(qkv, k_img, v_img, attn.heads, out_scale=scale, q_prescaled=True)
            st.hidden, h_stats = residual_gate_stats(st.hidden, o.view(st.hidden.shape))
            st.stats = ((h_stats, st.stats[0][1]), st.stats[1])
            return
        dim = attn.heads * attn.head_dim
        shp = (1, -1, attn.heads, attn.head_dim)
        o = F.scaled_dot_product_attention(qkv[:, :dim].contiguous().view(shp).transpose(1, 2), k_img.view(shp).transpose(1, 2),
                                           v_img.view(shp).transpose(1, 2), attn_mask=None, dropout_p=0.0, is_causal=False)
        st.hidden = st.hidden + scale * o.transpose(1, 2).reshape(1, -1, dim)
        if st.fused:  # (fused blocks around a torch-op adapter step: attention impl "sdpa" or a head dim other than 128)
            st.stats = ((residual_gate_stats(st.hidden)[1], st.stats[0][1]), st.stats[1])

    # True: the PuLID step runs the folded kernel (svdq_pulid_ca) and one residual pass; False: the reference's torch-op sequence
    pulid_fused = True

    def _pulid_check(self, hidden_states) -> None:
        """the refusals of a step with ``id_embeddings`` (before anything is launched)"""
        from ..caching import teacache

        if getattr(self, "pulid_ca", None) is None or len(self.pulid_ca) == 0:
            raise ValueError("id_embeddings were passed but no PuLID modules are attached: call models.pulid.attach_pulid(transformer, source) first")
        if hidden_states.shape[0] != 1:
            raise ValueError(f"PuLID supports batch 1 only (got {hidden_states.shape[0]}): run the samples one by one")
        if getattr(self, "_is_cached", False) and getattr(self, "residual_diff_threshold_multi", -1.0) >= 0.0:
            raise NotImplementedError("PuLID with First-Block Cache active is not supported: a skipped block's identity residual would be "
                                      "dropped (switch the cache off: residual_diff_threshold_multi < 0)")
        if any(hasattr(self, name) for name in teacache.STATE):
            raise NotImplementedError("PuLID inside a TeaCache context is not supported")
        if getattr(self, "offload", False):
            raise NotImplementedError("PuLID does not support an offloaded model")
        want = (len(self.blocks) + 1) // 2 + (len(self.single_blocks) + 3) // 4
        if len(self.pulid_ca) != want:
            raise ValueError(f"{len(self.pulid_ca)} PuLID modules are attached, the transformer needs {want}")

    def _pulid_add(self, st: "_Step", k: int) -> None:
        """``image rows += id_weight * pulid_ca[k](id_embeddings, image rows)`` (reference: FluxModel.cpp ``residual_callback``, behind the
        ControlNet add).  Fused arm: ``svdq_pulid_ca`` on the un-normalised rows (its own eps = 1e-5 statistics: one stats-only pass), then
        ONE ``svdq_residual_gate_stats`` pass that adds the result in place and renews the statistics the next block's quantisers read --
        in the joined stream the image rows' slice of them, as ``add_control`` does there.  Padded image rows take part like any row."""
        mods, emb, weight, fused = st.pulid
        t_pad = st.p_txt if st.joined else 0
        img = st.hidden[:, t_pad:]
        if fused:
            o = mods[k].forward_fused(emb, img, out_scale=weight)
            _, h_stats = residual_gate_stats(img, o)
            if st.joined:
                st.stats[0][t_pad:] = h_stats
            else:
                st.stats = ((h_stats, st.stats[0][1]), st.stats[1])
            return
        new = img + weight * mods[k](emb if emb.dim() == 3 else emb[None], img)
        if st.joined:
            st.hidden = torch.cat([st.hidden[:, :t_pad], new], dim=1)
        else:
            st.hidden = new
        if st.fused:  # (fused blocks around a torch-op PuLID step)
            h_stats = residual_gate_stats(new)[1]
            if st.joined:
                st.stats[0][t_pad:] = h_stats
            else:
                st.stats = ((h_stats, st.stats[0][1]), st.stats[1])

    def _join(self, st: "_Step") -> None:
        """[text | image] for the single blocks; the statistics in the same row order."""
        st.hidden = torch.cat([st.enc, st.hidden], dim=1)
        st.stats = (torch.cat([st.stats[1][0], st.stats[0][0]], dim=0), None) if st.fused else None  # [txt; img] row order
        st.joined = True

    def _run_single(self, st: "_Step", lo: int, hi: int, keep_input: bool = False) -> None:
        """Single blocks ``lo .. hi - 1`` on the joined stream; ``keep_input`` as in :meth:`_run_joint`."""
        ns, t_pad = len(self.single_blocks), st.p_txt
        for i in range(lo, hi):
            st.hidden, st.stats = self.single_blocks[i](st.hidden, st.temb_act, st.rot[2], st.stats, mods=st.mods.get(("s", i)),
                                                        kv_valid=st.kv_valid, keep_input=keep_input and i == lo)
            if st.cn_single is not None:
                _, i_stats = blocks.add_control(st.hidden[:, t_pad:], st.cn_single, i, ns, st.cn_repeat, want_stats=st.fused)
                if st.fused:
                    st.stats[0][t_pad:] = i_stats
            if st.pulid is not None and i % 4 == 0:
                self._pulid_add(st, (len(self.blocks) + 1) // 2 + i // 4)

    def _tail(self, st: "_Step") -> torch.Tensor:
        """The real image rows through AdaLayerNormContinuous and the output projection."""
        off = st.p_txt if st.joined else 0
        return self.proj_out(self.norm_out(st.hidden[:, off:off + st.t_img], st.temb_act))

    def _first_residual(self, name: str, curs, bases) -> torch.Tensor:
        """What the first block did to the real rows ``curs`` (one or two row ranges; ``bases``: the same rows before the block) as one
        ``[1, rows, dim]`` tensor -- and, in the same launch, its distance to the stored first residual ``name`` (handed to
        ``fbcache.are_two_tensors_similar`` with the tensor)."""
        from ..caching import fbcache

        prev = fbcache.get_buffer(name)
        out = torch.empty(1, sum(c.shape[0] for c in curs), self.dim, dtype=curs[0].dtype, device=curs[0].device)
        edges = [0]
        for c in curs:
            edges.append(edges[-1] + c.shape[0])
        cut = lambda t: [t[0, a:b] for a, b in zip(edges[:-1], edges[1:])]
        usable = prev is not None and prev.shape == out.shape and prev.dtype == out.dtype and prev.device == out.device and prev.is_contiguous()
        _, record = residual_diff(list(curs), list(bases), cut(prev) if usable else None, cut(out))
        return fbcache.attach_comparison(out, prev, record) if usable else out

    def engine_forward_cached(self, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None,
                              controlnet_block_samples=None, controlnet_single_block_samples=None, *, use_double_fb_cache: bool = False,
                              residual_diff_threshold_multi: float = 0.12, residual_diff_threshold_single: float = -1.0,
                              verbose: bool = False, ip_hidden_states=None):
        """One denoising step with First-Block Cache (reference: caching/utils_v2.py ``cached_forward_v2``): the stages of
        :meth:`engine_forward` with the decision of ``caching.fbcache.check_and_apply_cache`` in between.

        Behind joint block 0 the change it made to the real image rows is compared with the one of the last computed step
        (``svdq_residual_diff``: subtraction and comparison in one pass).  Hit: the other blocks are skipped and the stored residuals of
        the image and the text stream are added (one grouped ``svdq_residual_gate_stats`` pass); only block 0's modulation projections were
        launched.  Miss: the other blocks run and their summed effect is stored.  ``use_double_fb_cache``: the miss / hit above covers the
        joint blocks only and a second decision is taken behind single block 0 on the real rows of ``[text | image]``.

        Needs an active ``fbcache.cache_context``.  The decision is read on the host, which synchronises the stream.  Refused with an
        error: a stream under capture (``graph.CapturedStep``), batch > 1 (the uncached forward loops over the samples; one cache context
        holds one sample's residuals) and ControlNet residuals (the reference's cached forward drops them silently).

        With an IP-Adapter attached (``ip_hidden_states`` as in :meth:`engine_forward`) the adapter's step runs behind every joint block
        that runs: block 0's residual -- what the decision compares -- includes the adapter's contribution, as in the reference's
        ``IPA_TransformerBlocks``, and a hit launches no image-prompt attention beyond block 0's."""
        from ..caching import fbcache

        if hidden_states.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("First-Block Cache reads its decision on the host, which synchronises the stream: a cached forward cannot be "
                               "captured into a graph (run the uncached forward under capture: residual_diff_threshold_multi < 0)")
        if hidden_states.shape[0] != 1:
            raise ValueError(f"First-Block Cache supports batch 1 only (got {hidden_states.shape[0]}): run the samples one by one, each in "
                             "its own cache context")
        if controlnet_block_samples is not None or controlnet_single_block_samples is not None:
            raise ValueError("First-Block Cache does not support ControlNet residuals: the skipped blocks' residuals would be dropped")
        assert fbcache.get_current_cache_context() is not None, "cache_context must be set before"
        nj, ns = len(self.blocks), len(self.single_blocks)
        if nj == 0:
            raise ValueError("First-Block Cache needs at least one joint block")
        double = bool(use_double_fb_cache) and ns > 0

        st = self._prologue(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance,
                            ip_hidden_states=ip_hidden_states)
        t_txt, t_img, p_txt = st.t_txt, st.t_img, st.p_txt
        self._launch_mods(st, range(0, 1), range(0, 1) if double else range(0))  # of the blocks that run whatever the decision
        h0 = st.hidden
        self._run_joint(st, 0, 1, keep_input=True)
        first = self._first_residual("first_multi_hidden_states_residual", [st.hidden[0, :t_img]], [h0[0, :t_img]])
        del h0

        def apply_residual(hidden_states, encoder_hidden_states, mode):
            """a hit: the stored residuals are added in place; in double mode the same pass delivers single block 0's LayerNorm statistics"""
            if mode == "multi":
                h_res, e_res = fbcache.get_buffer("multi_hidden_states_residual"), fbcache.get_buffer("multi_encoder_hidden_states_residual")
                assert h_res is not None, "multi_hidden_states_residual must be set before"
                assert e_res is not None, "multi_encoder_hidden_states_residual must be set before"
                h_stats, e_stats = residual_add_pair(hidden_states, h_res, encoder_hidden_states, e_res, want_stats=double and st.fused)
                if double and st.fused:
                    st.stats = ((h_stats, None), (e_stats, None))
                return hidden_states, encoder_hidden_states
            res = fbcache.get_buffer("single_hidden_states_residual")
            assert res is not None, "single_hidden_states_residual must be set before"
            return residual_gate_stats(hidden_states, res, want_stats=False)[0]

        def remaining_multi(hidden_states, encoder_hidden_states):
            """a miss: the other joint blocks (and, with one decision per step, all single blocks); block 0's outputs survive for the residuals"""
            self._launch_mods(st, range(1, nj), range(0) if double else range(ns))
            self._run_joint(st, 1, nj, keep_input=True)
            if double:
                cur_e, cur_h = st.enc, st.hidden
            else:
                self._join(st)  # a new tensor: the single blocks update it in place
                self._run_single(st, 0, ns)
                cur_e, cur_h = st.hidden[:, :p_txt], st.hidden[:, p_txt:]
            (e_res, h_res), _ = residual_diff([cur_e[0], cur_h[0]], [encoder_hidden_states[0], hidden_states[0]])
            return cur_h, cur_e, h_res.unsqueeze(0), e_res.unsqueeze(0)

        st.hidden, st.enc, _ = fbcache.check_and_apply_cache(
            first_residual=first, hidden_states=st.hidden, encoder_hidden_states=st.enc, threshold=residual_diff_threshold_multi,
            parallelized=False, mode="multi", verbose=verbose, call_remaining_fn=remaining_multi, remaining_kwargs={},
            apply_residual_fn=apply_residual)
        st.joined = False  # (after a miss with one decision per step the two streams are views of the joined tensor)
        if double:
            self._join(st)
            s0 = st.hidden
            self._run_single(st, 0, 1, keep_input=True)
            real = lambda t: [t[0, :t_txt], t[0, p_txt:p_txt + t_img]]  # the padding rows take no part in the decision
            first = self._first_residual("first_single_hidden_states_residual", real(st.hidden), real(s0))
            del s0

            def remaining_single(hidden_states, encoder_hidden_states):
                self._launch_mods(st, range(0), range(1, ns))
                self._run_single(st, 1, ns, keep_input=True)
                res, _ = residual_diff(st.hidden[0], hidden_states[0])
                return st.hidden, res.unsqueeze(0)

            st.hidden, _, _ = fbcache.check_and_apply_cache(
                first_residual=first, hidden_states=st.hidden, encoder_hidden_states=None, threshold=residual_diff_threshold_single,
                parallelized=False, mode="single", verbose=verbose, call_remaining_fn=remaining_single, remaining_kwargs={},
                apply_residual_fn=apply_residual)
        return self._tail(st)

    def teacache_forward(self, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None,
                         controlnet_block_samples=None, controlnet_single_block_samples=None, *, decide):
        """One denoising step with TeaCache (reference: caching/teacache.py ``teacache_forward``): the decision is taken BEFORE any block runs,
        from the AdaLayerNormZero-modulated input of joint block 0 on the real image rows.

        Behind the embedders one ``svdq_modulated_diff`` pass forms that modulated input -- from the image stream's LayerNorm statistics (the
        ones block 0 consumes anyway on the fused path) and block 0's ``shift_msa`` / ``scale_msa`` -- stores it over the previous step's
        (``self.previous_modulated_input``, one buffer kept across steps) and compares the two on the way.  ``decide(ratio_fn)`` is the state
        machine of ``caching.teacache`` -> ``(should_calc, refresh)``; it calls ``ratio_fn`` (the host read of the record: synchronises the
        stream) only on steps whose outcome is not forced.  ``refresh`` False is a step inside the ``skip_steps`` window: every block runs,
        ``previous_residual`` stays.  Skip: ``hidden += previous_residual`` on the real image rows and the tail -- no block, no modulation
        projection but block 0's.  Computed step: the uncached step's launches, then ``previous_residual = hidden_after_blocks -
        hidden_after_embed`` (image rows; one ``svdq_residual_diff`` subtraction into the kept buffer).

        Refused with an error: a stream under capture, batch > 1, ControlNet residuals, a model with First-Block Cache switched on, an
        offloaded model, a model with an IP-Adapter attached."""
        if getattr(self, "ip_adapter", None) is not None:
            raise NotImplementedError("TeaCache with an IP-Adapter attached is not supported (the reference has no such combination): "
                                      "detach the adapter (undo_all_mods_on_transformer) or use First-Block Cache")
        if hidden_states.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TeaCache reads its decision on the host, which synchronises the stream: a cached forward cannot be "
                               "captured into a graph (run the uncached forward under capture: TeaCache(..., enabled=False))")
        if hidden_states.shape[0] != 1:
            raise ValueError(f"TeaCache supports batch 1 only (got {hidden_states.shape[0]}): run the samples one by one, each in "
                             "its own TeaCache context")
        if controlnet_block_samples is not None or controlnet_single_block_samples is not None:
            raise ValueError("TeaCache does not support ControlNet residuals: a skipped step would drop them")
        if getattr(self, "_is_cached", False) and getattr(self, "residual_diff_threshold_multi", -1.0) >= 0.0:
            raise RuntimeError("TeaCache and First-Block Cache cannot be active on the same model: both decide which blocks of a step run "
                               "(switch First-Block Cache off: residual_diff_threshold_multi < 0)")
        if getattr(self, "offload", False):  # (no FLUX model of this library sets it today -- only Qwen-Image offloads; the guard is for the day one does)
            raise NotImplementedError("TeaCache does not support an offloaded model")
        nj, ns = len(self.blocks), len(self.single_blocks)
        if nj == 0:
            raise ValueError("TeaCache needs at least one joint block (the decision reads its modulation)")

        st = self._prologue(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance)
        t_img = st.t_img
        self._launch_mods(st, range(0, 1), range(0))  # of the block whose modulation the decision reads
        mods0 = st.mods.get(("j", 0))
        shift_msa, scale_msa = (mods0[0] if mods0 is not None else self.blocks[0].mod(st.temb_act)).view(6, -1)[:2]
        x = st.hidden[0, :t_img]  # padding rows take no part
        stats = st.stats[0][0][:t_img] if st.fused else residual_gate_stats(x)[1]
        buf = getattr(self, "previous_modulated_input", None)
        usable = buf is not None and buf.shape == x.shape and buf.dtype == x.dtype and buf.device == x.device
        if not usable:  # first step of a context (or a new token count): the buffers that are then kept across steps
            buf = torch.empty_like(x)
            self._teacache_scratch = modulated_diff_scratch(t_img, x.device)
        _, record = modulated_diff(x, stats, scale_msa, shift_msa, prev=buf if usable else None, out=buf, scratch=self._teacache_scratch)
        self.previous_modulated_input = buf

        def ratio():
            if record is None:
                raise RuntimeError("TeaCache: no modulated input of the previous step with this step's shape to compare with "
                                   "(the token count changed inside a run of num_steps steps)")
            return record.read()["ratio"]

        should_calc, refresh = decide(ratio)
        res = getattr(self, "previous_residual", None)
        if refresh and not should_calc:
            if res is None or res.shape != x.shape or res.dtype != x.dtype or res.device != x.device:
                raise RuntimeError("TeaCache: a step is to be skipped but no residual of a computed step with this step's shape is stored")
            residual_gate_stats(x, res, want_stats=False)  # hidden += previous_residual, one 16-bit add in place
            return self._tail(st)
        h0 = st.hidden
        self._launch_mods(st, range(1, nj), range(ns))
        self._run_joint(st, 0, nj, keep_input=refresh)  # (the fused path updates the stream in place otherwise)
        self._join(st)
        self._run_single(st, 0, ns)
        if refresh:
            if res is None or res.shape != x.shape or res.dtype != x.dtype or res.device != x.device:
                res = torch.empty_like(x)
            residual_diff(st.hidden[0, st.p_txt:st.p_txt + t_img], h0[0, :t_img], out=res)
            self.previous_residual = res
        return self._tail(st)


class _Step:
    """What one denoising step carries between the stages of :class:`FluxEngineMixin`: the two streams (``hidden`` is the joined
    ``[text | image]`` stream once ``joined``), the LayerNorm statistics that travel with them on the fused path, and the step's constants."""

    __slots__ = ("hidden", "enc", "stats", "temb_act", "rot", "kv_valid", "t_txt", "t_img", "p_txt", "fused", "mods", "joined",
                 "cn_joint", "cn_single", "cn_repeat", "ip", "pulid")


class FluxTransformerAMD(nn.Module, FluxEngineMixin):
    """One denoising step: ``forward(latents, text states, pooled text, timestep, guidance, ids)`` (stand-alone; no diffusers)."""

    def __init__(self, num_layers=19, num_single_layers=38, dim=3072, heads=24, in_channels=64,
                 joint_attention_dim=4096, pooled_projection_dim=768, rank=32, guidance_embeds=True,
                 axes_dims_rope=(16, 56, 56), torch_dtype=torch.bfloat16, device="cuda"):
        super().__init__()
        self._build_engine(num_layers, num_single_layers, dim, heads, in_channels, joint_attention_dim, pooled_projection_dim,
                           rank, guidance_embeds, axes_dims_rope, torch_dtype, device)

    def forward(self, hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance=None):
        return self.engine_forward(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance)
