"""Stable Diffusion XL: the quantised transformer blocks of its U-Net and ``NunchakuSDXLUNet2DConditionModel`` (reference:
nunchaku/models/unets/unet_sdxl.py and nunchaku/models/attention_processors/sdxl.py).

    unet = NunchakuSDXLUNet2DConditionModel.from_pretrained("svdq-int4_r32-sdxl.safetensors", device="cuda")

SDXL is a U-Net: convolutions and ResNet blocks stay diffusers' own 16-bit modules; what SVDQuant quantises are the
``BasicTransformerBlock`` s inside its ``Transformer2DModel`` s -- widths 640 (10 heads) and 1280 (20 heads), head dimension 64, text
condition 2048 wide.  Every module here is constructible from dimensions alone (no diffusers needed) or from the diffusers module it
replaces, under the reference's child and parameter names, so a checkpoint's ``...transformer_blocks.*`` tensors load ``strict=True`` after
:func:`convert_sdxl_state_dict`.

The attention processor replaces the reference's ``chunk`` + three ``view`` / ``transpose`` copies + SDPA by one ``ops.attention_d64`` launch
that reads the thirds of the QKV projection (or the outputs of ``to_q`` / ``to_k`` / ``to_v``) in place.

* With diffusers importable the U-Net class is a real ``UNet2DConditionModel`` subclass (``_patch_model`` + ``from_pretrained``).
* Without diffusers it is an ``nn.Module`` that builds and loads the quantised transformer blocks from the checkpoint's keys, under the
  checkpoint's own module paths, keeps the remaining tensors as ``unquantized_state_dict`` and raises on ``forward``.

``precision="fp4"`` / ``"nvfp4"`` raises: NVFP4 needs Blackwell's block-scaled mma.  Not built: GEGLU fused into the quantiser (its
``fuse_glu`` is SiLU on interleaved pairs), caching ``to_k`` / ``to_v`` of the text across denoising steps, the shifted ResNet convolutions
(the reference leaves them unused), attention masks."""

from __future__ import annotations

import json
import os
from types import SimpleNamespace
from typing import Any, Dict, Optional

import torch
import torch.nn.functional as F
from torch import nn

from ..ops.attention import attention_d64
from .linear import SVDQW4A4Linear
from .transformer_flux import NunchakuModelLoaderMixin

try:  # the guarded import the reference does unconditionally (unet_sdxl.py:12-22)
    from diffusers import UNet2DConditionModel as _DiffusersUNet
    from diffusers.models.attention import BasicTransformerBlock as _DiffusersBlock
    from diffusers.models.attention import FeedForward as _DiffusersFeedForward

    HAVE_DIFFUSERS = True
except Exception:  # ImportError, or a diffusers build that cannot import on this platform
    _DiffusersUNet = _DiffusersBlock = _DiffusersFeedForward = None
    HAVE_DIFFUSERS = False

SVD_RANK = 32
HEAD_DIM = 64
_NVFP4 = "NVFP4 checkpoints need Blackwell's block-scaled mma; use the int4 checkpoint on MI355X"


def _check_precision(precision):
    if precision in ("fp4", "nvfp4"):
        raise NotImplementedError(_NVFP4)
    if precision not in (None, "auto", "int4"):
        raise ValueError(f"precision must be 'auto', 'int4' or 'fp4', got {precision!r}")


class NunchakuSDXLFA2Processor:
    """reference: attention_processors/sdxl.py -- its call signature and order of operations; the attention itself is one
    ``ops.attention_d64`` launch on the projections' outputs in place."""

    def __call__(self, attn, hidden_states: torch.Tensor, encoder_hidden_states: Optional[torch.Tensor] = None,
                 attention_mask: Optional[torch.Tensor] = None, **cross_attention_kwargs):
        input_ndim = hidden_states.ndim
        if input_ndim == 4:
            batch_size, channel, height, width = hidden_states.shape
            hidden_states = hidden_states.view(batch_size, channel, height * width).transpose(1, 2)
        if attention_mask is not None:
            raise NotImplementedError("attention_mask is not supported")
        if not attn.is_cross_attention:
            qkv = attn.to_qkv(hidden_states)               # [B, T, 3 * dim]: the thirds are read where the GEMM wrote them
            dim = qkv.shape[-1] // 3
            query, key, value = qkv[..., :dim], qkv[..., dim:2 * dim], qkv[..., 2 * dim:]
        else:
            query, key, value = attn.to_q(hidden_states), attn.to_k(encoder_hidden_states), attn.to_v(encoder_hidden_states)
        hidden_states = attention_d64(query, key, value, attn.heads)  # [B, T, dim] token-major: what to_out[0]'s quantiser reads
        hidden_states = attn.to_out[0](hidden_states)
        hidden_states = attn.to_out[1](hidden_states)
        if input_ndim == 4:
            hidden_states = hidden_states.transpose(-1, -2).reshape(batch_size, channel, height, width)
        return hidden_states / attn.rescale_output_factor


class NunchakuSDXLAttention(nn.Module):
    """reference: unet_sdxl.py:35-121.  Self-attention: ``to_qkv`` (one fused ``SVDQW4A4Linear``); cross-attention: ``to_q`` quantised,
    ``to_k`` / ``to_v`` unquantised ``nn.Linear(cross_attention_dim, dim, bias=False)``; ``to_out = [SVDQW4A4Linear, Dropout]``.

    ``NunchakuSDXLAttention(dim, heads, cross_attention_dim=None, rank=32, torch_dtype=..., device=...)`` builds it from dimensions;
    ``NunchakuSDXLAttention(orig_attn, rank=...)`` from a diffusers ``Attention`` as the reference does (dtype and device are its)."""

    def __init__(self, dim, heads: int | None = None, cross_attention_dim: int | None = None, processor: str = "flashattn2", rank: int = SVD_RANK,
                 precision: str = "int4", torch_dtype: torch.dtype = torch.bfloat16, device: str | torch.device | None = None,
                 rescale_output_factor: float = 1.0):
        super().__init__()
        _check_precision(precision)
        kw = dict(rank=rank, precision="int4")
        if isinstance(dim, int):
            if heads is None or heads < 1 or dim % heads:
                raise ValueError(f"NunchakuSDXLAttention: dim={dim} is not a multiple of heads={heads}")
            self.is_cross_attention = cross_attention_dim is not None
            self.heads = heads
            self.rescale_output_factor = rescale_output_factor
            kw.update(torch_dtype=torch_dtype, device=device)
            if not self.is_cross_attention:
                self.to_qkv = SVDQW4A4Linear(dim, 3 * dim, bias=False, **kw)
            else:
                self.to_q = SVDQW4A4Linear(dim, dim, bias=False, **kw)
                self.to_k = nn.Linear(cross_attention_dim, dim, bias=False, dtype=torch_dtype, device=device)
                self.to_v = nn.Linear(cross_attention_dim, dim, bias=False, dtype=torch_dtype, device=device)
            self.to_out = nn.ModuleList([SVDQW4A4Linear(dim, dim, bias=True, **kw), nn.Dropout(0.0)])
        else:
            orig_attn = dim
            self.is_cross_attention = orig_attn.is_cross_attention
            self.heads = orig_attn.heads
            self.rescale_output_factor = orig_attn.rescale_output_factor
            q = orig_attn.to_q
            if not orig_attn.is_cross_attention:  # the fused QKV projection
                self.to_qkv = SVDQW4A4Linear(q.in_features, q.out_features + orig_attn.to_k.out_features + orig_attn.to_v.out_features,
                                             bias=q.bias is not None, torch_dtype=q.weight.dtype, device=q.weight.device, **kw)
            else:
                self.to_q = SVDQW4A4Linear.from_linear(q, **kw)
                self.to_k = orig_attn.to_k
                self.to_v = orig_attn.to_v
            self.to_out = orig_attn.to_out
            self.to_out[0] = SVDQW4A4Linear.from_linear(self.to_out[0], **kw)
        self.set_processor(processor)

    def forward(self, hidden_states: torch.Tensor, encoder_hidden_states: Optional[torch.Tensor] = None,
                attention_mask: Optional[torch.Tensor] = None, **cross_attention_kwargs) -> torch.Tensor:
        return self.processor(self, hidden_states=hidden_states, encoder_hidden_states=encoder_hidden_states, attention_mask=attention_mask,
                              **cross_attention_kwargs)

    def set_processor(self, processor: str):
        if processor == "flashattn2":
            self.processor = NunchakuSDXLFA2Processor()
        else:
            raise ValueError(f"Processor {processor} is not supported")


class NunchakuSDXLGEGLU(nn.Module):
    """diffusers' ``GEGLU`` with a quantised ``proj``: ``h, g = proj(x).chunk(2, -1); h * gelu(g)`` in the 16-bit dtype."""

    def __init__(self, proj: SVDQW4A4Linear):
        super().__init__()
        self.proj = proj

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        hidden_states, gate = self.proj(hidden_states).chunk(2, dim=-1)
        return hidden_states * F.gelu(gate)


class NunchakuSDXLFeedForward(_DiffusersFeedForward if HAVE_DIFFUSERS else nn.Module):
    """reference: unet_sdxl.py:124-158.  ``net = [GEGLU(proj = SVDQW4A4Linear(dim, 8 * dim)), Dropout, SVDQW4A4Linear(4 * dim, dim)]``;
    built from ``dim`` or from a diffusers ``FeedForward`` (whose GEGLU and linear give the sizes, dtype and device)."""

    def __init__(self, ff, rank: int = SVD_RANK, precision: str = "int4", torch_dtype: torch.dtype = torch.bfloat16,
                 device: str | torch.device | None = None):
        nn.Module.__init__(self)
        _check_precision(precision)
        kw = dict(rank=rank, precision="int4")
        if isinstance(ff, int):
            dim = ff
            proj = SVDQW4A4Linear(dim, 8 * dim, bias=True, torch_dtype=torch_dtype, device=device, **kw)
            out = SVDQW4A4Linear(4 * dim, dim, bias=True, torch_dtype=torch_dtype, device=device, **kw)
        else:
            net = list(ff.net)
            if len(net) < 3 or not isinstance(getattr(net[0], "proj", None), nn.Linear) or not isinstance(net[2], nn.Linear):
                raise ValueError("NunchakuSDXLFeedForward: expected a FeedForward whose net is [GEGLU, Dropout, Linear]")
            proj, out = SVDQW4A4Linear.from_linear(net[0].proj, **kw), SVDQW4A4Linear.from_linear(net[2], **kw)
        self.net = nn.ModuleList([NunchakuSDXLGEGLU(proj), nn.Dropout(0.0), out])

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        for module in self.net:
            hidden_states = module(hidden_states)
        return hidden_states


class NunchakuSDXLTransformerBlock(_DiffusersBlock if HAVE_DIFFUSERS else nn.Module):
    """reference: unet_sdxl.py:161-286.  ``NunchakuSDXLTransformerBlock(dim, heads, cross_attention_dim, rank=32, torch_dtype=..., device=...)``
    or ``NunchakuSDXLTransformerBlock(block, rank=...)`` from a diffusers ``BasicTransformerBlock`` (its norms are kept)."""

    def __init__(self, block, heads: int | None = None, cross_attention_dim: int | None = None, rank: int = SVD_RANK, precision: str = "int4",
                 torch_dtype: torch.dtype = torch.bfloat16, device: str | torch.device | None = None):
        nn.Module.__init__(self)
        _check_precision(precision)
        if isinstance(block, int):
            dim = block
            if cross_attention_dim is None:
                raise ValueError("NunchakuSDXLTransformerBlock: cross_attention_dim is required")
            kw = dict(rank=rank, torch_dtype=torch_dtype, device=device)
            self.norm_type, self.pos_embed, self.only_cross_attention = "layer_norm", None, False
            self.norm1 = nn.LayerNorm(dim, dtype=torch_dtype, device=device)
            self.norm2 = nn.LayerNorm(dim, dtype=torch_dtype, device=device)
            self.norm3 = nn.LayerNorm(dim, dtype=torch_dtype, device=device)
            self.attn1 = NunchakuSDXLAttention(dim, heads, **kw)
            self.attn2 = NunchakuSDXLAttention(dim, heads, cross_attention_dim, **kw)
            self.ff = NunchakuSDXLFeedForward(dim, **kw)
        else:
            self.norm_type = block.norm_type
            self.pos_embed = block.pos_embed
            self.only_cross_attention = block.only_cross_attention
            self.norm1, self.norm2, self.norm3 = block.norm1, block.norm2, block.norm3
            self.attn1 = NunchakuSDXLAttention(block.attn1, rank=rank)
            self.attn2 = NunchakuSDXLAttention(block.attn2, rank=rank)
            self.ff = NunchakuSDXLFeedForward(block.ff, rank=rank)

    def forward(self, hidden_states: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                encoder_hidden_states: Optional[torch.Tensor] = None, encoder_attention_mask: Optional[torch.Tensor] = None,
                timestep: Optional[torch.LongTensor] = None, cross_attention_kwargs: Dict[str, Any] = None,
                class_labels: Optional[torch.LongTensor] = None, added_cond_kwargs: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        if self.norm_type == "layer_norm":
            norm_hidden_states = self.norm1(hidden_states)
        else:
            raise ValueError("Incorrect norm used")
        if self.pos_embed is not None:
            norm_hidden_states = self.pos_embed(norm_hidden_states)
        cross_attention_kwargs = cross_attention_kwargs.copy() if cross_attention_kwargs is not None else {}
        gligen_kwargs = cross_attention_kwargs.pop("gligen", None)
        if self.only_cross_attention:
            raise ValueError("only_cross_attention cannot be True")
        attn_output = self.attn1(norm_hidden_states, encoder_hidden_states=None, attention_mask=attention_mask, **cross_attention_kwargs)
        hidden_states = attn_output + hidden_states
        if hidden_states.ndim == 4:
            hidden_states = hidden_states.squeeze(1)
        if gligen_kwargs is not None:
            hidden_states = self.fuser(hidden_states, gligen_kwargs["objs"])
        if self.attn2 is not None:
            if self.norm_type == "layer_norm":
                norm_hidden_states = self.norm2(hidden_states)
            else:
                raise ValueError("Incorrect norm")
            if self.pos_embed is not None and self.norm_type != "ada_norm_single":
                norm_hidden_states = self.pos_embed(norm_hidden_states)
            attn_output = self.attn2(norm_hidden_states, encoder_hidden_states=encoder_hidden_states, attention_mask=encoder_attention_mask,
                                     **cross_attention_kwargs)
            hidden_states = attn_output + hidden_states
        norm_hidden_states = self.norm3(hidden_states)
        ff_output = self.ff(norm_hidden_states)
        hidden_states = ff_output + hidden_states
        if hidden_states.ndim == 4:
            hidden_states = hidden_states.squeeze(1)
        return hidden_states


def convert_sdxl_state_dict(state_dict: dict[str, torch.Tensor]) -> dict[str, torch.Tensor]:
    """The checkpoint's names -> this package's, inside ``.transformer_blocks.`` only (reference: unet_sdxl.py:526-544): ``lora_down`` ->
    ``proj_down``, ``lora_up`` -> ``proj_up``, ``smooth_orig`` -> ``smooth_factor_orig``, ``smooth`` -> ``smooth_factor`` (``smooth_orig`` is
    looked for first: ``smooth`` is its prefix).  Names that are already converted and every other key pass through."""
    renames = ((".lora_down", ".proj_down"), (".lora_up", ".proj_up"), (".smooth_orig", ".smooth_factor_orig"), (".smooth", ".smooth_factor"))
    out = {}
    for k, v in state_dict.items():
        if ".transformer_blocks." in k and ".smooth_factor" not in k:
            for old, new in renames:
                if old in k:
                    k = k.replace(old, new)
                    break
        out[k] = v
    return out


_BLOCK_MARK = ".transformer_blocks."


def _block_prefixes(keys):
    """``down_blocks.1.attentions.0.transformer_blocks.0`` ... of the keys that lie in a transformer block, in first-seen order"""
    seen = {}
    for k in keys:
        i = k.find(_BLOCK_MARK)
        if i < 0:
            continue
        rest = k[i + len(_BLOCK_MARK):]
        seen.setdefault(k[:i + len(_BLOCK_MARK)] + rest.split(".", 1)[0], None)
    return list(seen)


_Base = _DiffusersUNet if HAVE_DIFFUSERS else nn.Module


class NunchakuSDXLUNet2DConditionModel(_Base, NunchakuModelLoaderMixin):
    """``StableDiffusionXLPipeline``'s ``unet`` with the quantised transformer blocks (reference: unet_sdxl.py:381-523)."""

    if HAVE_DIFFUSERS:

        def _patch_model(self, **kwargs):
            """Replace every ``BasicTransformerBlock`` of the down, up and mid blocks that carry attentions by a
            :class:`NunchakuSDXLTransformerBlock` (reference :386-466; its asserts)."""
            _check_precision(kwargs.get("precision", "int4"))
            rank = kwargs.get("rank", SVD_RANK)

            def _patch_attentions(block):
                for attn in block.attentions:
                    assert hasattr(attn, "transformer_blocks"), "Dual cross attention is not supported"
                    blocks = []
                    for transformer_block in attn.transformer_blocks:
                        assert isinstance(transformer_block, _DiffusersBlock)
                        blocks.append(NunchakuSDXLTransformerBlock(transformer_block, rank=rank))
                    attn.transformer_blocks = nn.ModuleList(blocks)

            for block in list(self.down_blocks) + list(self.up_blocks):
                if getattr(block, "attentions", None) is not None:  # CrossAttnDownBlock2D / CrossAttnUpBlock2D
                    _patch_attentions(block)
            assert getattr(self.mid_block, "attentions", None) is not None, "Only UNetMidBlock2DCrossAttn is supported"
            _patch_attentions(self.mid_block)
            return self

    else:  # ModelMixin provides these; the skeleton is made by _build_model

        @property
        def dtype(self) -> torch.dtype:
            return self.dtype_

        @property
        def device(self) -> torch.device:
            return next(self.parameters()).device

        def forward(self, *args, **kwargs):
            raise RuntimeError("NunchakuSDXLUNet2DConditionModel.forward: the convolutions, ResNet blocks, time and text embeddings of the U-Net "
                               "are diffusers' own modules and diffusers is not importable here; install diffusers, or run the quantised "
                               "blocks through model.transformer_block(name)(...)")

        def _patch_model(self, keys=(), shapes=None, **kwargs):
            """Build the quantised transformer blocks that the (converted) checkpoint names, each under the checkpoint's own module path;
            sizes come from the tensors' shapes: ``attn1.to_qkv.qweight`` [3 * dim, dim / 2], ``attn2.to_k.weight`` [dim, cross_dim]."""
            _check_precision(kwargs.get("precision", "int4"))
            rank, shapes = kwargs.get("rank", SVD_RANK), shapes or {}
            self.transformer_block_names = _block_prefixes(keys)
            for prefix in self.transformer_block_names:
                try:
                    dim = shapes[prefix + ".attn1.to_qkv.qweight"][1] * 2
                    cross = shapes[prefix + ".attn2.to_k.weight"][1]
                except KeyError as e:
                    raise ValueError(f"{prefix}: the checkpoint lacks {e.args[0]}: not a quantised SDXL transformer block") from None
                if prefix + ".attn1.to_qkv.proj_down" in shapes:
                    rank = shapes[prefix + ".attn1.to_qkv.proj_down"][1]
                block = NunchakuSDXLTransformerBlock(dim, dim // HEAD_DIM, cross, rank=rank, torch_dtype=self.dtype_, device=kwargs.get("device"))
                parent = self
                *path, last = prefix.split(".")
                for name in path:
                    if name not in parent._modules:
                        parent.add_module(name, nn.Module())
                    parent = parent._modules[name]
                parent.add_module(last, block)
            return self

        def transformer_block(self, name: str) -> NunchakuSDXLTransformerBlock:
            """the block at a checkpoint path such as ``down_blocks.1.attentions.0.transformer_blocks.0``"""
            return self.get_submodule(name)

    @classmethod
    def _build_model(cls, pretrained_model_name_or_path: str | os.PathLike, **kwargs):
        sd, meta = cls._read_safetensors(pretrained_model_name_or_path)
        config = json.loads(meta.get("config", "{}"))
        dtype = kwargs.get("torch_dtype", torch.bfloat16)
        if HAVE_DIFFUSERS:
            with torch.device("meta"):  # the skeleton only: to_empty materialises it after the blocks are patched
                unet = cls.from_config(config)
        else:
            unet = cls.__new__(cls)
            nn.Module.__init__(unet)
            unet.config = SimpleNamespace(**config)
            unet.dtype_ = dtype
        return unet, sd, meta

    @classmethod
    def from_pretrained(cls, pretrained_model_path: str | os.PathLike, **kwargs):
        """A nunchaku ``.safetensors`` file, local or ``org/repo/file`` on the hub; ``device`` (default "cpu", as the reference), ``torch_dtype``,
        ``precision`` ("auto" | "int4"; "fp4" raises); ``offload=True`` raises (reference :468-523)."""
        device = kwargs.get("device", "cpu")
        if kwargs.get("offload", False):
            raise NotImplementedError("Offload is not supported for NunchakuSDXLUNet2DConditionModel")
        _check_precision(kwargs.get("precision", "auto"))
        torch_dtype = kwargs.get("torch_dtype", torch.bfloat16)
        unet, sd, meta = cls._build_model(pretrained_model_path, **kwargs)
        qcfg = json.loads(meta.get("quantization_config", "{}"))
        if any(k.endswith(".wcscales") for k in sd) or qcfg.get("weight", {}).get("dtype", "int4") not in ("int4",):
            raise NotImplementedError(_NVFP4)
        rank = qcfg.get("rank", SVD_RANK)
        converted = convert_sdxl_state_dict(sd)
        if HAVE_DIFFUSERS:
            unet = unet.to(torch_dtype)
            unet._patch_model(precision="int4", rank=rank)
            unet = unet.to_empty(device=device)
            unet.load_state_dict(converted)
        else:
            quantized = {k: v for k, v in converted.items() if _BLOCK_MARK in k}
            unet._patch_model(keys=quantized, shapes={k: tuple(v.shape) for k, v in quantized.items()}, precision="int4", rank=rank, device=device)
            unet.load_state_dict(quantized, strict=True)
            unet.unquantized_state_dict = {k: v for k, v in converted.items() if _BLOCK_MARK not in k}
        return unet
