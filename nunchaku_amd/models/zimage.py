"""Z-Image(-Turbo): the quantised single-stream blocks and ``NunchakuZImageTransformer2DModel`` (reference:
nunchaku/models/transformers/transformer_zimage.py and nunchaku/models/attention_processors/zimage.py).

    transformer = NunchakuZImageTransformer2DModel.from_pretrained("svdq-int4_r32-z-image-turbo.safetensors", device="cuda")

A Z-Image block is ``x += tanh(gate) * norm2(attention(norm1(x) * (1 + scale)))`` and the same around a SwiGLU feed-forward: four full-width
RMSNorms, two per-sample modulations and two gated residuals around two sub-layers, a per-head RMSNorm of Q and K and a RoPE inside the
attention.  Every linear layer (dim 3840: 3840 -> 11520, 3840 -> 3840, 3840 -> 20480, 10240 -> 3840) is an ``SVDQW4A4Linear``.  The glue runs in
two kernels of its own:

* ``ops.sandwich_norm`` (``svdq_sandwich_norm``): one row pass closes a sub-layer (RMSNorm of its output, gate, residual) and opens the next
  (RMSNorm of the sum, modulation).  :class:`ZImageBlockStack` hands the pass behind a feed-forward the NEXT block's ``attention_norm1`` and
  scale, so a stack of N blocks launches 2 N + 1 of them.
* ``ops.qk_norm_rope`` (``svdq_qk_norm_rope``): per sample, the two per-head RMSNorms and the rotation of the packed QKV projection in place
  and V transposed, which is what ``ops.attention.attention_packed`` (``svdq_attention``, head dimension 128, key-padding mask) reads.  The
  token axis is padded to a multiple of 128 rows once per stack; the padding rows are zeros and their keys are masked.

Every module is constructible from dimensions alone (no diffusers needed) under the reference's child and parameter names, so a checkpoint's
``layers.*`` / ``noise_refiner.*`` / ``context_refiner.*`` tensors load ``strict=True``.

* With diffusers importable the model class is a real ``ZImageTransformer2DModel`` subclass (``_patch_model`` + ``from_pretrained``) whose blocks
  keep diffusers' forward; their attention runs through :class:`NunchakuZSingleStreamAttnProcessor`.
* Without diffusers it is an ``nn.Module`` that builds the quantised blocks from the checkpoint's keys under the checkpoint's module paths, keeps
  the remaining tensors as ``unquantized_state_dict``, offers the three stacks (``stack("layers")``) and raises on ``forward``.

Not built: SwiGLU folded into the quantiser's ``fuse_glu`` (DESIGN.md 6p prices it), Q pre-scaling for the attention's second geometry, a batched
QK launch, caching the modulation across blocks, a LoRA converter, NVFP4 (``precision="fp4"`` raises), offload (raises as in the reference)."""

from __future__ import annotations

import json
import os
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from ..ops.attention import attention_packed, qk_norm_rope
from ..ops.elementwise import sandwich_norm
from .linear import SVDQW4A4Linear
from .transformer_flux import NunchakuModelLoaderMixin

try:  # the guarded import the reference does unconditionally (transformer_zimage.py:11-14)
    from diffusers.models.transformers.transformer_z_image import ZImageTransformer2DModel as _DiffusersZImage

    HAVE_DIFFUSERS = True
except Exception:  # ImportError, or a diffusers build without Z-Image
    _DiffusersZImage = None
    HAVE_DIFFUSERS = False

SVD_RANK = 32
HEAD_DIM = 128
NORM_EPS = 1e-5
ADALN_EMBED_DIM = 256
STACKS = ("noise_refiner", "context_refiner", "layers")
_NVFP4 = "NVFP4 checkpoints need Blackwell's block-scaled mma; use the int4 checkpoint on MI355X"


def _check_precision(precision):
    if precision in ("fp4", "nvfp4"):
        raise NotImplementedError(_NVFP4)
    if precision not in (None, "auto", "int4"):
        raise ValueError(f"precision must be 'auto', 'int4' or 'fp4', got {precision!r}")


def _pad128(n: int) -> int:
    return (n + 127) // 128 * 128


def valid_token_counts(attention_mask: Optional[torch.Tensor], B: int, T: int) -> list[int]:
    """The real tokens per sample of a 2-D boolean mask whose real tokens come first (None: all T are real).  Reads the mask on the host."""
    if attention_mask is None:
        return [T] * B
    m = attention_mask
    if not isinstance(m, torch.Tensor) or m.dim() != 2 or m.dtype != torch.bool or tuple(m.shape) != (B, T):
        raise NotImplementedError(f"Z-Image attention: attention_mask must be a boolean [{B}, {T}] key-padding mask, got "
                                  f"{getattr(m, 'dtype', type(m).__name__)} {tuple(getattr(m, 'shape', ()))}")
    counts = m.sum(dim=1)
    if not bool((m == (torch.arange(T, device=m.device)[None, :] < counts[:, None])).all()):
        raise NotImplementedError("Z-Image attention: the real tokens of every sample must come first in attention_mask")
    counts = [int(n) for n in counts.tolist()]
    if min(counts) < 1:
        raise ValueError("Z-Image attention: a sample without real tokens")
    return counts


class NunchakuZSingleStreamAttnProcessor:
    """reference: attention_processors/zimage.py -- its call signature and order of operations.  ``to_qkv``, then per sample one
    ``ops.qk_norm_rope`` launch (both norms, the rotation, V transposed) and one ``ops.attention.attention_packed`` launch on the packed buffer,
    then ``to_out``."""

    def attend_padded(self, attn, hidden_states: torch.Tensor, counts: list[int], freqs_cis: Optional[torch.Tensor]) -> torch.Tensor:
        """``hidden_states`` ``[B, L, C]`` with L a multiple of 128, sample b's first ``counts[b]`` rows real -> ``to_out[0]`` of the attention,
        ``[B, L, C]`` (the rows behind a sample's real ones attend to its real keys: finite, and nobody's business)"""
        B, L, C = hidden_states.shape
        dev, dt = hidden_states.device, hidden_states.dtype
        qkv = torch.empty(B, L, 3 * C, dtype=dt, device=dev)
        attn.to_qkv(hidden_states, output=qkv.view(B * L, 3 * C))
        vt = torch.empty(B, C, L, dtype=dt, device=dev)
        out = torch.empty(B, L, C, dtype=dt, device=dev)
        wq = attn.norm_q.weight if attn.norm_q is not None else None
        wk = attn.norm_k.weight if attn.norm_k is not None else None
        eps = attn.norm_q.eps if attn.norm_q is not None else attn.norm_k.eps if attn.norm_k is not None else NORM_EPS
        for b, n in enumerate(counts):  # one sample per launch: Z-Image-Turbo runs batch 1
            qk_norm_rope(qkv[b], attn.heads, n, norm_q=wq, norm_k=wk, freqs_cis=None if freqs_cis is None else freqs_cis[b, :n], vt=vt[b],
                         eps=NORM_EPS if eps is None else eps)
            attention_packed(qkv[b], vt[b], attn.heads, out=out[b], kv_valid=(n,) if n < L else None)
        return attn.to_out[0](out)

    def __call__(self, attn, hidden_states: torch.Tensor, encoder_hidden_states: Optional[torch.Tensor] = None,
                 attention_mask: Optional[torch.Tensor] = None, freqs_cis: Optional[torch.Tensor] = None) -> torch.Tensor:
        B, T, C = hidden_states.shape
        counts = valid_token_counts(attention_mask, B, T)
        L = _pad128(T)
        if L != T or min(counts) < T:  # the padded buffer of the attention: zeros behind every sample's real rows
            padded = hidden_states.new_zeros(B, L, C)
            for b, n in enumerate(counts):
                padded[b, :n] = hidden_states[b, :n]
        else:
            padded = hidden_states
        output = self.attend_padded(attn, padded, counts, freqs_cis)[:, :T]
        if len(attn.to_out) > 1:  # dropout
            output = attn.to_out[1](output)
        return output


class NunchakuZImageAttention(nn.Module):
    """reference: transformer_zimage.py:27-116.  ``to_qkv`` (one fused ``SVDQW4A4Linear``, no bias), ``norm_q`` / ``norm_k``
    (``RMSNorm(128, eps=1e-5)``), ``to_out = [SVDQW4A4Linear (no bias), Dropout]``.

    ``NunchakuZImageAttention(dim, heads, rank=32, torch_dtype=..., device=...)`` builds it from dimensions;
    ``NunchakuZImageAttention(orig_attn, rank=...)`` from a diffusers ``Attention`` as the reference does (dtype and device are its)."""

    def __init__(self, dim, heads: int | None = None, processor: str = "flashattn2", rank: int = SVD_RANK, precision: str = "int4",
                 torch_dtype: torch.dtype = torch.bfloat16, device: str | torch.device | None = None):
        super().__init__()
        _check_precision(precision)
        kw = dict(rank=rank, precision="int4")
        if isinstance(dim, int):
            if heads is None or heads < 1 or dim != heads * HEAD_DIM:
                raise ValueError(f"NunchakuZImageAttention: dim={dim} is not heads={heads} x {HEAD_DIM}")
            self.heads = heads
            self.inner_dim = self.query_dim = self.out_dim = dim
            self.use_bias, self.dropout, self.is_cross_attention, self.rescale_output_factor = False, 0.0, False, 1.0
            kw.update(torch_dtype=torch_dtype, device=device)
            self.norm_q = nn.RMSNorm(HEAD_DIM, eps=NORM_EPS, dtype=torch_dtype, device=device)
            self.norm_k = nn.RMSNorm(HEAD_DIM, eps=NORM_EPS, dtype=torch_dtype, device=device)
            self.to_qkv = SVDQW4A4Linear(dim, 3 * dim, bias=False, **kw)
            self.to_out = nn.ModuleList([SVDQW4A4Linear(dim, dim, bias=False, **kw), nn.Dropout(0.0)])
        else:
            orig_attn = dim
            for name in ("inner_dim", "query_dim", "use_bias", "dropout", "out_dim", "heads", "rescale_output_factor", "is_cross_attention"):
                setattr(self, name, getattr(orig_attn, name))
            self.norm_q, self.norm_k = orig_attn.norm_q, orig_attn.norm_k
            q = orig_attn.to_q
            self.to_qkv = SVDQW4A4Linear(q.in_features, q.out_features + orig_attn.to_k.out_features + orig_attn.to_v.out_features,
                                         bias=q.bias is not None, torch_dtype=q.weight.dtype, device=q.weight.device, **kw)
            self.to_out = orig_attn.to_out
            self.to_out[0] = SVDQW4A4Linear.from_linear(self.to_out[0], **kw)
        self.set_processor(processor)

    def forward(self, hidden_states: torch.Tensor, encoder_hidden_states: Optional[torch.Tensor] = None,
                attention_mask: Optional[torch.Tensor] = None, **cross_attention_kwargs) -> torch.Tensor:
        return self.processor(attn=self, hidden_states=hidden_states, encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask,
                              **cross_attention_kwargs)

    def set_processor(self, processor: str):
        if processor == "flashattn2":
            self.processor = NunchakuZSingleStreamAttnProcessor()
        else:
            raise ValueError(f"Processor {processor} is not supported")


class NunchakuZImageSwiGLU(nn.Module):
    """diffusers' ``SwiGLU`` with a quantised ``proj``: ``value, gate = proj(x).chunk(2, -1); value * silu(gate)`` in the 16-bit dtype."""

    def __init__(self, proj: SVDQW4A4Linear):
        super().__init__()
        self.proj = proj

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        hidden_states, gate = self.proj(hidden_states).chunk(2, dim=-1)
        return hidden_states * F.silu(gate)


class NunchakuZImageFeedForward(nn.Module):
    """reference: transformer_zimage.py:119-166 -- Z-Image's ``w2(silu(w1 x) * w3 x)`` as diffusers' SwiGLU ``FeedForward``, quantised the way
    ``NunchakuSDXLFeedForward`` is: ``net = [SwiGLU(proj = SVDQW4A4Linear(dim, 2 * hidden)), Dropout, SVDQW4A4Linear(hidden, dim)]``, no biases.
    Built from ``(dim, hidden)`` or from a diffusers Z-Image ``FeedForward`` (whose ``w1`` / ``w2`` give the sizes, dtype and device)."""

    def __init__(self, ff, hidden: int | None = None, rank: int = SVD_RANK, precision: str = "int4", torch_dtype: torch.dtype = torch.bfloat16,
                 device: str | torch.device | None = None):
        super().__init__()
        _check_precision(precision)
        if not isinstance(ff, int):
            w1, w2, w3 = ff.w1, ff.w2, ff.w3
            if (w1.in_features, w1.out_features) != (w3.in_features, w3.out_features) or w1.out_features != w2.in_features:
                raise ValueError("NunchakuZImageFeedForward: expected a Z-Image FeedForward with w1 / w3 [hidden, dim] and w2 [dim, hidden]")
            ff, hidden, torch_dtype, device = w1.in_features, w2.in_features, w1.weight.dtype, w1.weight.device
        if hidden is None or hidden < 1:
            raise ValueError("NunchakuZImageFeedForward: hidden is required")
        kw = dict(rank=rank, precision="int4", bias=False, torch_dtype=torch_dtype, device=device)
        self.net = nn.ModuleList([NunchakuZImageSwiGLU(SVDQW4A4Linear(ff, 2 * hidden, **kw)), nn.Dropout(0.0), SVDQW4A4Linear(hidden, ff, **kw)])

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        for module in self.net:
            hidden_states = module(hidden_states)
        return hidden_states


class ZImageSwiGLUFeedForward(nn.Module):
    """What the reference's ``_convert_z_image_ff`` makes of a Z-Image ``FeedForward`` that stays unquantised (the refiners under ``skip_refiners``):
    diffusers' SwiGLU ``FeedForward`` -- ``net = [SwiGLU(proj = Linear(dim, 2 * hidden)), Dropout, Linear(hidden, dim)]``, no biases -- with
    uninitialised parameters: such a checkpoint holds the refiners' feed-forwards under these names."""

    def __init__(self, ff):
        super().__init__()
        w1, w2 = ff.w1, ff.w2
        kw = dict(bias=False, dtype=w1.weight.dtype, device=w1.weight.device)
        self.net = nn.ModuleList([NunchakuZImageSwiGLU(nn.Linear(w1.in_features, 2 * w1.out_features, **kw)), nn.Dropout(0.0),
                                  nn.Linear(w2.in_features, w2.out_features, **kw)])

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        for module in self.net:
            hidden_states = module(hidden_states)
        return hidden_states


class NunchakuZImageTransformerBlock(nn.Module):
    """diffusers' ``ZImageTransformerBlock`` with the reference's quantised ``attention`` and ``feed_forward``:
    ``NunchakuZImageTransformerBlock(dim, heads, hidden, modulation=True, rank=32, torch_dtype=..., device=...)``.  ``forward`` runs the fused
    path of a one-block :class:`ZImageBlockStack`."""

    def __init__(self, dim: int, heads: int, hidden: int, modulation: bool = True, rank: int = SVD_RANK, precision: str = "int4",
                 norm_eps: float = NORM_EPS, adaln_dim: int | None = None, torch_dtype: torch.dtype = torch.bfloat16,
                 device: str | torch.device | None = None):
        super().__init__()
        _check_precision(precision)
        kw = dict(rank=rank, torch_dtype=torch_dtype, device=device)
        self.dim, self.head_dim, self.modulation = dim, dim // heads, modulation
        self.attention = NunchakuZImageAttention(dim, heads, **kw)
        self.feed_forward = NunchakuZImageFeedForward(dim, hidden, **kw)
        nkw = dict(eps=norm_eps, dtype=torch_dtype, device=device)
        self.attention_norm1, self.ffn_norm1 = nn.RMSNorm(dim, **nkw), nn.RMSNorm(dim, **nkw)
        self.attention_norm2, self.ffn_norm2 = nn.RMSNorm(dim, **nkw), nn.RMSNorm(dim, **nkw)
        if modulation:
            adaln_dim = min(dim, ADALN_EMBED_DIM) if adaln_dim is None else adaln_dim
            self.adaLN_modulation = nn.Sequential(nn.Linear(adaln_dim, 4 * dim, bias=True, dtype=torch_dtype, device=device))

    def modulate(self, adaln_input: Optional[torch.Tensor]):
        """``(1 + scale_msa, tanh(gate_msa), 1 + scale_mlp, tanh(gate_mlp))``, each ``[B, dim]`` in the 16-bit dtype; Nones without modulation"""
        if not self.modulation:
            return None, None, None, None
        if adaln_input is None:
            raise ValueError("NunchakuZImageTransformerBlock: a block with modulation needs adaln_input")
        scale_msa, gate_msa, scale_mlp, gate_mlp = self.adaLN_modulation(adaln_input).chunk(4, dim=-1)
        return 1.0 + scale_msa, gate_msa.tanh(), 1.0 + scale_mlp, gate_mlp.tanh()

    def forward(self, x: torch.Tensor, attn_mask: Optional[torch.Tensor], freqs_cis: Optional[torch.Tensor],
                adaln_input: Optional[torch.Tensor] = None) -> torch.Tensor:
        return ZImageBlockStack([self])(x, attn_mask, freqs_cis, adaln_input)


class ZImageBlockStack:
    """The fused path over a sequence of :class:`NunchakuZImageTransformerBlock` s (a ``ModuleList``, or any slice of one).  The tokens are
    copied once into ``[B, L, C]`` buffers, L the next multiple of 128 (zeros behind every sample's real rows); per block there are two
    ``ops.sandwich_norm`` launches -- behind the attention, which also opens the feed-forward, and behind the feed-forward, which also opens the
    NEXT block's attention with that block's ``attention_norm1`` and scale -- and per sample one ``ops.qk_norm_rope`` and one attention launch;
    one opening pass per stack."""

    def __init__(self, blocks):
        self.blocks = list(blocks)
        if not self.blocks:
            raise ValueError("ZImageBlockStack: no blocks")

    def __call__(self, x: torch.Tensor, attn_mask: Optional[torch.Tensor] = None, freqs_cis: Optional[torch.Tensor] = None,
                 adaln_input: Optional[torch.Tensor] = None) -> torch.Tensor:
        if x.dim() != 3:
            raise ValueError(f"ZImageBlockStack: x must be [B, T, C], got {tuple(x.shape)}")
        B, T, C = x.shape
        counts = valid_token_counts(attn_mask, B, T)
        if freqs_cis is not None and tuple(freqs_cis.shape[:2]) != (B, T):
            raise ValueError(f"ZImageBlockStack: freqs_cis must be [{B}, {T}, 64], got {tuple(freqs_cis.shape)}")
        L = _pad128(T)
        h = x.new_zeros(B, L, C)
        for b, n in enumerate(counts):
            h[b, :n] = x[b, :n]
        blk = self.blocks[0]
        mod = blk.modulate(adaln_input)
        _, hm, _ = sandwich_norm(h, None, w_pre=blk.attention_norm1.weight, scale=mod[0], out=False, out_mod=True, eps=blk.attention_norm1.eps)
        for i, blk in enumerate(self.blocks):
            nxt = self.blocks[i + 1] if i + 1 < len(self.blocks) else None
            a = blk.attention.processor.attend_padded(blk.attention, hm, counts, freqs_cis)
            sandwich_norm(h, a, w_post=blk.attention_norm2.weight, gate=mod[1], w_pre=blk.ffn_norm1.weight, scale=mod[2], out=h, out_mod=hm,
                          eps=blk.ffn_norm1.eps)
            f = blk.feed_forward(hm)
            gate_mlp = mod[3]
            if nxt is not None:
                mod = nxt.modulate(adaln_input)
                sandwich_norm(h, f, w_post=blk.ffn_norm2.weight, gate=gate_mlp, w_pre=nxt.attention_norm1.weight, scale=mod[0], out=h, out_mod=hm,
                              eps=blk.ffn_norm2.eps)
            else:
                sandwich_norm(h, f, w_post=blk.ffn_norm2.weight, gate=gate_mlp, out=h, out_mod=False, eps=blk.ffn_norm2.eps)
        return h[:, :T]


def patch_scale_key(transformer: nn.Module, state_dict: dict) -> None:
    """What the reference's helper of this name does before ``load_state_dict`` (transformers/utils.py:151-173): a ``wcscales`` the model has
    and the checkpoint lacks becomes ones, every other tensor must be there with the model's kind of dtype, and a layer's ``wtscale`` (a Python float,
    not a parameter) is taken out of the checkpoint."""
    own = transformer.state_dict()
    for k, v in own.items():
        if k not in state_dict:
            if ".wcscales" not in k:
                raise KeyError(f"the checkpoint lacks {k}")
            state_dict[k] = torch.ones_like(v)
        elif v.is_floating_point() != state_dict[k].is_floating_point():  # (bf16 <-> fp16 is load_state_dict's cast, as for the other models)
            raise TypeError(f"{k}: the checkpoint holds {state_dict[k].dtype}, the model {v.dtype}")
    for n, m in transformer.named_modules():
        if isinstance(m, SVDQW4A4Linear) and getattr(m, "wtscale", None) is not None:
            m.wtscale = state_dict.pop(f"{n}.wtscale", 1.0)


def _block_prefixes(keys):
    """``layers.0`` ... of the keys that lie in a quantised block of one of the three stacks, in numeric order per stack"""
    seen = set()
    for k in keys:
        parts = k.split(".")
        if len(parts) > 2 and parts[0] in STACKS and parts[1].isdigit() and k.endswith(".attention.to_qkv.qweight"):
            seen.add((STACKS.index(parts[0]), int(parts[1])))
    return [f"{STACKS[s]}.{i}" for s, i in sorted(seen)]


_Base = _DiffusersZImage if HAVE_DIFFUSERS else nn.Module


class NunchakuZImageTransformer2DModel(_Base, NunchakuModelLoaderMixin):
    """``ZImagePipeline``'s ``transformer`` with the quantised blocks (reference: transformer_zimage.py:169-269)."""

    if HAVE_DIFFUSERS:

        def _patch_model(self, skip_refiners: bool = False, **kwargs):
            """Replace ``attention`` and ``feed_forward`` of every block of ``layers`` and, unless ``skip_refiners``, of the two refiners
            (reference :174-208; with ``skip_refiners`` the refiners keep their 16-bit attention and get the SwiGLU form of their feed-forward)."""
            _check_precision(kwargs.get("precision", "int4"))
            rank = kwargs.get("rank", SVD_RANK)
            for blocks in (self.layers, self.noise_refiner, self.context_refiner):
                for block in blocks:
                    if skip_refiners and blocks is not self.layers:
                        block.feed_forward = ZImageSwiGLUFeedForward(block.feed_forward)
                        continue
                    block.attention = NunchakuZImageAttention(block.attention, rank=rank)
                    block.feed_forward = NunchakuZImageFeedForward(block.feed_forward, rank=rank)
            return self

    else:  # ModelMixin provides these; the skeleton is made by _build_model

        @property
        def dtype(self) -> torch.dtype:
            return self.dtype_

        @property
        def device(self) -> torch.device:
            return next(self.parameters()).device

        def forward(self, *args, **kwargs):
            raise RuntimeError("NunchakuZImageTransformer2DModel.forward: the patch embedders, the timestep and caption embedders, the rotary "
                               "embedder and the final layer of Z-Image are diffusers' own modules and diffusers is not importable here; install "
                               "diffusers, or run the quantised blocks through model.stack(name)(x, attn_mask, freqs_cis, adaln_input)")

        def _patch_model(self, keys=(), shapes=None, skip_refiners: bool = False, **kwargs):
            """Build the quantised blocks that the checkpoint names, each under the checkpoint's own module path; sizes come from the tensors'
            shapes: ``attention.to_qkv.qweight`` [3 * dim, dim / 2], ``feed_forward.net.2.qweight`` [dim, hidden / 2],
            ``adaLN_modulation.0.weight`` [4 * dim, embed] (absent: a block without modulation)."""
            _check_precision(kwargs.get("precision", "int4"))
            rank, shapes = kwargs.get("rank", SVD_RANK), shapes or {}
            self.block_names = [p for p in _block_prefixes(keys) if not (skip_refiners and not p.startswith("layers."))]
            for prefix in self.block_names:
                try:
                    dim = shapes[prefix + ".attention.to_qkv.qweight"][1] * 2
                    hidden = shapes[prefix + ".feed_forward.net.2.qweight"][1] * 2
                except KeyError as e:
                    raise ValueError(f"{prefix}: the checkpoint lacks {e.args[0]}: not a quantised Z-Image block") from None
                if prefix + ".attention.to_qkv.proj_down" in shapes:
                    rank = shapes[prefix + ".attention.to_qkv.proj_down"][1]
                adaln = shapes.get(prefix + ".adaLN_modulation.0.weight")
                block = NunchakuZImageTransformerBlock(dim, dim // HEAD_DIM, hidden, modulation=adaln is not None, rank=rank,
                                                       norm_eps=getattr(self.config, "norm_eps", NORM_EPS), adaln_dim=adaln[1] if adaln else None,
                                                       torch_dtype=self.dtype_, device=kwargs.get("device"))
                stack, index = prefix.split(".")
                if stack not in self._modules:
                    self.add_module(stack, nn.ModuleList())
                if int(index) != len(self._modules[stack]):
                    raise ValueError(f"{prefix}: the blocks of {stack} are not numbered 0 .. n - 1 in the checkpoint")
                self._modules[stack].append(block)
            return self

        def stack(self, name: str) -> ZImageBlockStack:
            """the fused path over ``layers``, ``noise_refiner`` or ``context_refiner``"""
            if name not in STACKS or name not in self._modules:
                raise KeyError(f"{name}: this model has the quantised stacks {[s for s in STACKS if s in self._modules]}")
            return ZImageBlockStack(self._modules[name])

    @classmethod
    def _build_model(cls, pretrained_model_name_or_path: str | os.PathLike, **kwargs):
        sd, meta = cls._read_safetensors(pretrained_model_name_or_path)
        config = json.loads(meta.get("config", "{}"))
        dtype = kwargs.get("torch_dtype", torch.bfloat16)
        if HAVE_DIFFUSERS:
            with torch.device("meta"):  # the skeleton only: to_empty materialises it after the blocks are patched
                transformer = cls.from_config(config)
        else:
            transformer = cls.__new__(cls)
            nn.Module.__init__(transformer)
            transformer.config = SimpleNamespace(**config)
            transformer.dtype_ = dtype
        return transformer, sd, meta

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str | os.PathLike, **kwargs):
        """A nunchaku ``.safetensors`` file, local or ``org/repo/file`` on the hub; ``device`` (default "cpu", as the reference), ``torch_dtype``,
        ``precision`` ("auto" | "int4"; "fp4" raises); ``offload=True`` raises.  The metadata's ``quantization_config`` gives ``rank`` and
        ``skip_refiners`` (reference :210-269)."""
        device = kwargs.get("device", "cpu")
        if kwargs.get("offload", False):
            raise NotImplementedError("Offload is not supported for ZImageTransformer2DModel")
        _check_precision(kwargs.get("precision", "auto"))
        torch_dtype = kwargs.get("torch_dtype", torch.bfloat16)
        transformer, sd, meta = cls._build_model(pretrained_model_name_or_path, **kwargs)
        qcfg = json.loads(meta.get("quantization_config", "{}"))
        if qcfg.get("weight", {}).get("dtype", "int4") not in ("int4",):
            raise NotImplementedError(_NVFP4)
        rank, skip_refiners = qcfg.get("rank", SVD_RANK), bool(qcfg.get("skip_refiners", False))
        if HAVE_DIFFUSERS:
            transformer = transformer.to(torch_dtype)
            transformer._patch_model(skip_refiners=skip_refiners, precision="int4", rank=rank)
            transformer = transformer.to_empty(device=device)
            patch_scale_key(transformer, sd)
            transformer.load_state_dict(sd)
        else:
            transformer._patch_model(keys=sd, shapes={k: tuple(v.shape) for k, v in sd.items()}, skip_refiners=skip_refiners, precision="int4",
                                     rank=rank, device=device)
            own = tuple(p + "." for p in transformer.block_names)
            quantized = {k: v for k, v in sd.items() if k.startswith(own)}
            patch_scale_key(transformer, quantized)
            transformer.load_state_dict(quantized, strict=True)
            transformer.unquantized_state_dict = {k: v for k, v in sd.items() if not k.startswith(own)}
        return transformer
