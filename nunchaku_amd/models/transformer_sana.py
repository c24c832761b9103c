"""``NunchakuSanaTransformer2DModel``: diffusers' ``SanaTransformer2DModel`` with its ``transformer_blocks`` replaced by the quantised stack
(reference: nunchaku/models/transformers/transformer_sana.py).

    transformer = NunchakuSanaTransformer2DModel.from_pretrained("svdq-int4_r32-sana1.6b.safetensors", pag_layers=8)

* With diffusers importable the class is a real ``SanaTransformer2DModel`` subclass: ``_build_model`` makes the diffusers skeleton from the
  checkpoint's ``config`` on the meta device, ``inject_quantized_module`` replaces ``transformer_blocks`` by ONE
  :class:`NunchakuSanaTransformerBlocks` (diffusers' forward then calls it once, with its per-block argument list), the remaining modules --
  patch embedding, ``AdaLayerNormSingle``, caption projection, the final modulated norm -- stay diffusers' own and take the rest of the file.
* Without diffusers it is an ``nn.Module`` that holds ``transformer_blocks`` and keeps the remaining tensors as ``unquantized_state_dict``;
  the quantised stack runs (``model.transformer_blocks[0](...)``), the full latent-to-latent ``forward`` raises and names diffusers.

``precision="fp4"`` raises: NVFP4 needs Blackwell's block-scaled mma."""

from __future__ import annotations

import json
import os
from types import SimpleNamespace

import torch
import torch.nn.functional as F
from torch import nn

from .sana import SanaModel, convert_sana_state_dict
from .transformer_flux import NunchakuModelLoaderMixin

try:  # the guarded import the reference does unconditionally (transformer_sana.py:11)
    from diffusers import SanaTransformer2DModel as _DiffusersSana

    HAVE_DIFFUSERS = True
except Exception:  # ImportError, or a diffusers build that cannot import on this platform / has no SANA
    _DiffusersSana = None
    HAVE_DIFFUSERS = False

SVD_RANK = 32
MASK_THRESHOLD = -9000  # an additive attention mask: real tokens are 0, padding is -10000 (transformer_sana.py:97)

# diffusers' SanaTransformer2DModel defaults are SANA-1.6B's
_DEFAULT_CONFIG = dict(in_channels=32, out_channels=32, num_attention_heads=70, attention_head_dim=32, num_layers=20, num_cross_attention_heads=20,
                       cross_attention_head_dim=112, cross_attention_dim=2240, caption_channels=2304, mlp_ratio=2.5, patch_size=1, sample_size=32)


def mask_key_counts(encoder_attention_mask: torch.Tensor, batch_size: int, txt_tokens: int):
    """``(mask [B, L], key_counts int32 [B], cu_seqlens_txt int32 [B + 1])`` of the additive mask ``[B, 1, L]`` diffusers passes, with the
    reference's expressions (transformer_sana.py:93-99).  No host synchronisation."""
    if encoder_attention_mask is None or tuple(encoder_attention_mask.shape) != (batch_size, 1, txt_tokens):
        raise ValueError(f"encoder_attention_mask must be [{batch_size}, 1, {txt_tokens}], got "
                         f"{None if encoder_attention_mask is None else tuple(encoder_attention_mask.shape)}")
    mask = encoder_attention_mask.reshape(batch_size, txt_tokens)
    counts = (mask > MASK_THRESHOLD).sum(dim=1)
    cu_seqlens_txt = F.pad(counts.cumsum(dim=0), pad=(1, 0), value=0).to(torch.int32)
    return mask, counts.to(torch.int32), cu_seqlens_txt


def token_grid(img_tokens: int, height: int | None, width: int | None):
    """the reference's derivation of the token grid (transformer_sana.py:104-110)"""
    if height is None and width is None:
        height = width = int(img_tokens ** 0.5)
    elif height is None:
        height = img_tokens // width
    elif width is None:
        width = img_tokens // height
    if height * width != img_tokens:
        raise ValueError(f"a grid of {height} x {width} does not hold {img_tokens} tokens")
    return height, width


class NunchakuSanaTransformerBlocks(nn.Module):
    """The quantised stack behind the argument list of a diffusers SANA block (reference: transformer_sana.py:25-214): ``pag`` is
    ``batch_size % 3 == 0`` and ``cfg`` is True, as there.

    By default the padded condition ``[B, L, dim]`` and ``key_counts = (mask > -9000).sum(1)`` go to ``SanaModel.forward_padded``: no boolean
    index, no host synchronisation, capturable.  This ASSUMES that a sample's real tokens come first and its padding behind them (what a
    tokenizer with right padding gives and diffusers' SANA pipeline passes): a mask with holes would select the first ``count`` tokens, not the
    unmasked ones.  ``pack_condition=True`` follows the reference literally -- ``encoder_hidden_states[mask > -9000]`` and ``cu_seqlens_txt``,
    a boolean index that synchronises -- and is right for any mask."""

    def __init__(self, m: SanaModel, dtype: torch.dtype, device: str | torch.device, pack_condition: bool = False):
        super().__init__()
        self.m = m
        self.dtype = dtype
        self.device = torch.device(device)
        self.pack_condition = bool(pack_condition)

    def _call(self, idx, hidden_states, encoder_hidden_states, encoder_attention_mask, timestep, height, width, skip_first_layer=False):
        batch_size, img_tokens = hidden_states.shape[:2]
        txt_tokens = encoder_hidden_states.shape[1]
        original_dtype, original_device = hidden_states.dtype, hidden_states.device
        mask, key_counts, cu_seqlens_txt = mask_key_counts(encoder_attention_mask, batch_size, txt_tokens)
        height, width = token_grid(img_tokens, height, width)
        pag, cfg = batch_size % 3 == 0, True  # (the reference's: pag is set when the model is loaded; CFG is not detected)
        x = hidden_states.to(self.dtype).to(self.device)
        t = timestep.to(self.dtype).to(self.device)
        cond = encoder_hidden_states.to(self.dtype).to(self.device)
        if self.pack_condition:
            cu_seqlens_img = torch.arange(0, (batch_size + 1) * img_tokens, img_tokens, dtype=torch.int32, device=self.device)
            args = (x, cond[mask.to(self.device) > MASK_THRESHOLD], t, cu_seqlens_img, cu_seqlens_txt.to(self.device), height, width, pag, cfg)
            out = self.m.forward(*args, skip_first_layer) if idx is None else self.m.forward_layer(idx, *args)
        else:
            args = (x, cond, t, key_counts.to(self.device), height, width, pag, cfg)
            out = self.m.forward_padded(*args, skip_first_layer) if idx is None else self.m.forward_layer_padded(idx, *args)
        return out.to(original_dtype).to(original_device)

    def forward(self, hidden_states: torch.Tensor, attention_mask: torch.Tensor | None = None, encoder_hidden_states: torch.Tensor | None = None,
                encoder_attention_mask: torch.Tensor | None = None, timestep: torch.Tensor | None = None, height: int | None = None,
                width: int | None = None, skip_first_layer: bool | None = False):
        """hidden_states [B, T, dim], encoder_hidden_states [B, L, dim], encoder_attention_mask [B, 1, L] (additive), timestep [B, 6 * dim]
        -> [B, T, dim] after all blocks (``skip_first_layer``: after blocks 1 ..); ``attention_mask`` is not used, as in the reference."""
        return self._call(None, hidden_states, encoder_hidden_states, encoder_attention_mask, timestep, height, width, bool(skip_first_layer))

    def forward_layer_at(self, idx: int, hidden_states: torch.Tensor, attention_mask: torch.Tensor | None = None,
                         encoder_hidden_states: torch.Tensor | None = None, encoder_attention_mask: torch.Tensor | None = None,
                         timestep: torch.Tensor | None = None, height: int | None = None, width: int | None = None):
        """block ``idx`` alone (what a first-block cache needs)"""
        return self._call(int(idx), hidden_states, encoder_hidden_states, encoder_attention_mask, timestep, height, width)


def load_quantized_module(net, path_or_state_dict, device: str | torch.device = "cuda", pag_layers: int | list[int] | None = None,
                          use_fp4: bool = False, rank: int = SVD_RANK) -> SanaModel:
    """A :class:`SanaModel` for ``net.config`` (and ``net.dtype``) with the ``transformer_blocks.*`` tensors of a state dict, or of a
    ``.safetensors`` file, loaded ``strict=True`` after :func:`convert_sana_state_dict` (reference: transformer_sana.py:308-350)."""
    if use_fp4:
        raise NotImplementedError("NVFP4 checkpoints need Blackwell's block-scaled mma; use the int4 checkpoint on MI355X")
    if not isinstance(path_or_state_dict, dict):
        path_or_state_dict, _ = NunchakuModelLoaderMixin._read_safetensors(path_or_state_dict)
    sd = convert_sana_state_dict({k: v for k, v in path_or_state_dict.items() if k.startswith("transformer_blocks.")})
    if any(k.endswith(".wcscales") for k in sd):
        raise NotImplementedError("NVFP4 checkpoints need Blackwell's block-scaled mma; use the int4 checkpoint on MI355X")
    dtype = getattr(net, "dtype", torch.bfloat16)
    m = SanaModel(net.config, pag_layers, rank=rank, torch_dtype=dtype, device=device)
    m.load_state_dict(sd, strict=True)
    return m


def inject_quantized_module(net, m: SanaModel, device: str | torch.device = "cuda"):
    """reference: transformer_sana.py:353-374"""
    net.transformer_blocks = nn.ModuleList([NunchakuSanaTransformerBlocks(m, net.dtype, device)])
    return net


_Base = _DiffusersSana if HAVE_DIFFUSERS else nn.Module


class NunchakuSanaTransformer2DModel(_Base, NunchakuModelLoaderMixin):
    """``SanaPipeline``'s ``transformer`` with the quantised blocks (reference: transformer_sana.py:217-305)."""

    if not HAVE_DIFFUSERS:  # ModelMixin provides these; the skeleton is made by _build_model (nn.Module.__init__ + config)

        @property
        def dtype(self) -> torch.dtype:
            return self.dtype_

        @property
        def device(self) -> torch.device:
            return self.transformer_blocks[0].device

        def forward(self, *args, **kwargs):
            raise RuntimeError("NunchakuSanaTransformer2DModel.forward: the patch embedding, AdaLayerNormSingle, the caption projection and the final "
                               "modulated norm are diffusers' own modules and diffusers is not importable here; install diffusers, or run the "
                               "quantised blocks through model.transformer_blocks[0](...)")

    @classmethod
    def _build_model(cls, pretrained_model_name_or_path: str | os.PathLike, **kwargs):
        sd, meta = cls._read_safetensors(pretrained_model_name_or_path)
        config = json.loads(meta.get("config", "{}"))
        dtype = kwargs.get("torch_dtype", torch.bfloat16)
        if HAVE_DIFFUSERS:
            with torch.device("meta"):  # the skeleton only: the blocks are replaced, the rest is materialised by to_empty
                transformer = cls.from_config(config).to(dtype)
        else:
            transformer = cls.__new__(cls)
            nn.Module.__init__(transformer)
            cfg = dict(_DEFAULT_CONFIG)
            cfg.update(config)
            transformer.config = SimpleNamespace(**cfg)
            transformer.dtype_ = dtype
        return transformer, sd, meta

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str | os.PathLike, **kwargs):
        """A nunchaku ``.safetensors`` file, local or ``org/repo/file`` on the hub; ``device``, ``pag_layers``, ``precision`` ("auto" | "int4";
        "fp4" raises), ``torch_dtype``, ``return_metadata`` (reference :225-286; its legacy folder layout is not read)."""
        device = torch.device(kwargs.get("device", "cuda"))
        precision = kwargs.get("precision", "auto")
        if precision == "fp4":
            raise NotImplementedError("NVFP4 checkpoints need Blackwell's block-scaled mma; use the int4 checkpoint on MI355X")
        if precision not in ("auto", "int4"):
            raise ValueError(f"precision must be 'auto', 'int4' or 'fp4', got {precision!r}")
        transformer, sd, meta = cls._build_model(pretrained_model_name_or_path, **kwargs)
        qcfg = json.loads(meta.get("quantization_config", "{}"))
        if qcfg.get("weight", {}).get("dtype", "int4") not in ("int4",):
            raise NotImplementedError("NVFP4 checkpoints need Blackwell's block-scaled mma; use the int4 checkpoint on MI355X")
        quantized = {k: v for k, v in sd.items() if k.startswith("transformer_blocks.")}
        unquantized = {k: v for k, v in sd.items() if not k.startswith("transformer_blocks.")}
        m = load_quantized_module(transformer, quantized, device=device, pag_layers=kwargs.get("pag_layers", []), rank=qcfg.get("rank", SVD_RANK))
        transformer.inject_quantized_module(m, device)
        if HAVE_DIFFUSERS:
            blocks = transformer.transformer_blocks  # (already on the device: to_empty would drop their contents)
            transformer.transformer_blocks = nn.ModuleList()
            transformer.to_empty(device=device)
            transformer.transformer_blocks = blocks
            transformer.load_state_dict(unquantized, strict=False)
        else:
            transformer.unquantized_state_dict = unquantized
        return (transformer, meta) if kwargs.get("return_metadata", False) else transformer

    def inject_quantized_module(self, m: SanaModel, device: str | torch.device = "cuda"):
        """reference :288-305"""
        self.transformer_blocks = nn.ModuleList([NunchakuSanaTransformerBlocks(m, self.dtype, device)])
        return self
