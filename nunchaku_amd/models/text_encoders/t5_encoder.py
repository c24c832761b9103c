"""NunchakuT5EncoderModel: the 4-bit (AWQ W4A16, group 128) T5 text encoder of the FLUX pipelines, loaded from one local
``.safetensors`` file (role of the reference's ``nunchaku/models/text_encoders/t5_encoder.py``).  Every ``nn.Linear`` with a
``<name>.qweight`` entry in the file becomes a :class:`W4Linear`; everything else is transformers' ``T5EncoderModel``, except its attention:
on a GPU, at ``d_kv == 64``, the encoder's self-attention runs as one ``ops.attention_d64_bias`` launch per layer (:func:`fused_t5_attention`,
registered with transformers' attention-function registry under :data:`ATTENTION_NAME`; ``T5Attention.forward`` itself is not touched).
transformers is imported when this module is."""

import json
import os

import torch
from torch import nn
from transformers import T5Config, T5EncoderModel
from transformers.models.t5.modeling_t5 import T5Block, T5LayerNorm

from .linear import W4Linear

__all__ = ["NunchakuT5EncoderModel", "ATTENTION_NAME", "fused_t5_attention", "toeplitz_rel_bias", "FusedT5Block", "FusedT5LayerNorm"]

ATTENTION_NAME = "nunchaku_amd_t5_d64"  # the name ``config._attn_implementation`` carries when the fused attention is selected

# tied embedding of T5EncoderModel: a file that stores one of the two names serves both
_TIED = ("shared.weight", "encoder.embed_tokens.weight")


def _read_safetensors(path: str) -> tuple[dict, dict]:
    from safetensors import safe_open

    tensors = {}
    with safe_open(path, framework="pt", device="cpu") as f:
        meta = f.metadata() or {}
        for k in f.keys():
            tensors[k] = f.get_tensor(k)
    return tensors, meta


def toeplitz_rel_bias(position_bias: torch.Tensor) -> torch.Tensor:
    """The float32 ``[H, T + N - 1]`` vector per head behind a ``[1, H, T, N]`` position bias that depends on ``key - query`` only
    (``T5Attention.compute_bias``): entry ``d + T - 1`` holds the bias of distance ``d`` -- column 0 reversed (d = -(T-1) .. -1), then row 0
    (d = 0 .. N-1).  Built once per tensor and version (the 24 layers of an encoder share one position bias)."""
    from ..._C import _cached_conversion

    def build(pb):
        return torch.cat((pb[0, :, 1:, 0].flip(-1), pb[0, :, 0, :]), dim=-1).float().contiguous()

    return _cached_conversion(position_bias, "t5_toeplitz", build)


def _key_bias(mask, B: int, N: int):
    """``(True, key_bias)`` for a mask the kernel takes -- None, ``[B, 1, 1, N]``, or ``[B, 1, T, N]`` expanded along T (stride 0): float32
    ``[B, N]`` or None; ``(False, None)`` for any other mask (it may vary along queries or heads)."""
    if mask is None:
        return True, None
    if (not isinstance(mask, torch.Tensor) or mask.dim() != 4 or not mask.is_floating_point() or mask.shape[0] != B or mask.shape[1] != 1
            or mask.shape[3] != N or not (mask.shape[2] == 1 or mask.stride(2) == 0)):
        return False, None
    from ..._C import _cached_conversion

    return True, _cached_conversion(mask, "t5_key_bias", lambda m: m[:, 0, 0, :].float().contiguous())


def _serves(module, query, key, value, attention_mask, dropout, position_bias) -> bool:
    """whether the kernel serves this call, from shapes, strides, dtypes and flags alone (the device is the caller's question)"""
    B, H, T, D = query.shape
    N = key.shape[2]
    return bool(D == 64 and not getattr(module, "is_decoder", False) and not (module.training and dropout > 0.0)
                and query.dtype in (torch.bfloat16, torch.float16) and key.dtype == query.dtype and value.dtype == query.dtype
                and isinstance(position_bias, torch.Tensor) and tuple(position_bias.shape) == (1, H, T, N) and tuple(value.shape) == tuple(key.shape)
                and not (torch.is_grad_enabled() and (query.requires_grad or key.requires_grad or value.requires_grad or position_bias.requires_grad))
                # [B, H, rows, 64] views of token-major [B, rows, H * 64] projections
                and all(t.stride(3) == 1 and (H == 1 or t.stride(1) == 64) for t in (query, key, value))
                and _key_bias(attention_mask, B, N)[0])


def fused_t5_attention(module, query, key, value, attention_mask, scaling=None, dropout=0.0, position_bias=None, **kwargs):
    """An attention function for transformers' registry (the signature of its ``eager_attention_forward``): the T5 encoder's self-attention as one
    ``ops.attention_d64_bias`` launch.  ``query`` / ``key`` / ``value`` are the ``[B, H, T, 64]`` transposed views of the projections' outputs:
    they are taken back to their token-major ``[B, T, H * 64]`` rows without a copy; the ``[1, H, T, N]`` position bias becomes its Toeplitz
    vector (:func:`toeplitz_rel_bias`), a padding mask the kernel's ``key_bias``.  Returns ``([B, T, H, 64], None)``.
    Everything else goes to transformers' own eager function, unchanged: a CPU tensor, ``d_kv != 64``, a decoder, training with dropout or
    with gradients, a mask that varies along queries or heads, a position bias that is not ``[1, H, T, N]``, projections that are not
    token-major rows.
    One visible difference from the eager function: a sample whose padding mask leaves NO key (``finfo(bfloat16).min`` on every key) comes out
    as exact zeros here, where eager's softmax over ``finfo.min + score`` gives a weighting of the padded keys."""
    if not (query.is_cuda and _serves(module, query, key, value, attention_mask, dropout, position_bias)):
        from transformers.models.t5.modeling_t5 import eager_attention_forward

        return eager_attention_forward(module, query, key, value, attention_mask, scaling=scaling, dropout=dropout, position_bias=position_bias,
                                       **kwargs)
    from ...ops.attention import attention_d64_bias

    B, H, T, _ = query.shape
    rows = [t.transpose(1, 2) for t in (query, key, value)]
    q, k, v = (r.flatten(2) if r.stride(2) == 64 else r.reshape(B, -1, H * 64) for r in rows)
    out = attention_d64_bias(q, k, v, H, toeplitz_rel_bias(position_bias), _key_bias(attention_mask, B, key.shape[2])[1],
                             scale=1.0 if scaling is None else scaling)
    return out.unflatten(-1, (H, 64)), None


def _padding_mask(batch_size, q_length, kv_length, q_offset=0, kv_offset=0, mask_function=None, attention_mask=None, dtype=torch.float32,
                  use_vmap=False, **kwargs):
    """The mask function that goes with :data:`ATTENTION_NAME` (transformers drops the mask of an attention name it has no mask function
    for): a 2-D padding mask of a bidirectional encoder becomes the additive ``[B, 1, 1, N]`` tensor -- 0 / ``finfo(dtype).min`` -- it is, not
    the ``[B, 1, T, N]`` copies of it that the eager mask function materialises; no mask stays None.  Anything else is the eager mask function's."""
    from transformers.masking_utils import bidirectional_mask_function, eager_mask

    if (mask_function is bidirectional_mask_function and not use_vmap and isinstance(q_offset, int) and q_offset == 0
            and isinstance(kv_offset, int) and kv_offset == 0):
        if attention_mask is None:
            return None
        if attention_mask.dim() == 2 and tuple(attention_mask.shape) == (batch_size, kv_length):
            keep = attention_mask.to(torch.bool)[:, None, None, :]
            return torch.where(keep, torch.zeros((), dtype=dtype, device=keep.device), torch.finfo(dtype).min)
    return eager_mask(batch_size=batch_size, q_length=q_length, kv_length=kv_length, q_offset=q_offset, kv_offset=kv_offset,
                      mask_function=mask_function, attention_mask=attention_mask, dtype=dtype, use_vmap=use_vmap, **kwargs)


def register_fused_attention() -> bool:
    """Put :func:`fused_t5_attention` and its mask function into transformers' registries; False when the installed transformers has none
    (the model then runs transformers' eager attention, as before)."""
    try:
        from transformers.masking_utils import ALL_MASK_ATTENTION_FUNCTIONS, bidirectional_mask_function, eager_mask  # noqa: F401
        from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS
        from transformers.models.t5.modeling_t5 import eager_attention_forward  # noqa: F401
    except ImportError:
        return False
    if ATTENTION_NAME not in ALL_ATTENTION_FUNCTIONS:
        ALL_ATTENTION_FUNCTIONS.register(ATTENTION_NAME, fused_t5_attention)
        ALL_MASK_ATTENTION_FUNCTIONS.register(ATTENTION_NAME, _padding_mask)
    return True


class FusedT5LayerNorm(T5LayerNorm):
    """``T5LayerNorm`` as one ``ops.t5_residual_norm`` launch (the stack's ``final_layer_norm`` under ``set_fused_layers``); same parameter,
    same rounding points.  What the kernel does not serve goes to the parent's forward."""

    def forward(self, hidden_states):
        w = self.weight
        if not (hidden_states.is_cuda and hidden_states.dtype in (torch.bfloat16, torch.float16) and w.dtype == hidden_states.dtype
                and hidden_states.shape[-1] % 8 == 0 and hidden_states.is_contiguous() and not (torch.is_grad_enabled() and (hidden_states.requires_grad or w.requires_grad))):
            return super().forward(hidden_states)
        from ...ops.elementwise import t5_residual_norm

        return t5_residual_norm(hidden_states, None, w.data, self.variance_epsilon)[1]


class FusedT5Block(T5Block):
    """A ``T5Block`` of the 4-bit encoder on the fused kernels (``set_fused_layers``): the class of an existing block is swapped, its children
    -- and with them the ``state_dict()`` keys -- stay.  One layer is

        norm (first layer only) -> q / k / v as ONE ``gemm_awq_multi`` launch into ``[B, T, 3 * inner]`` -> ``attention_d64_bias`` on its column
        thirds in place -> o -> ``y = hidden + o`` and the feed-forward norm in one ``t5_residual_norm`` pass -> ``gelu_new(wi_0) * wi_1`` as ONE
        gated ``gemm_awq_multi`` launch -> wo -> the closing add, with the NEXT layer's norm in the same pass (handed over through
        ``_next`` / ``_handed``; the last layer hands nothing, the stack's final norm is a :class:`FusedT5LayerNorm`).

    In float16 ``T5Block``'s inf-clamp sits between an add and the norm behind it: it stays the torch operations it is, and add and norm run as
    two passes.  Whatever :meth:`_serves` does not admit -- a CPU tensor, training, gradients, a decoder, ``d_kv != 64``, a feed-forward that
    is not gated-GELU on group-128 ``W4Linear`` children, a mask or position bias the attention kernel does not take -- goes to the parent's
    forward, per call."""

    _next = None    # the following block when it is fused too (a plain attribute set by set_fused_layers, not a registered child)
    _handed = None  # (hidden_states, its norm for this block) from the previous block's closing pass

    def _serves(self, hidden_states, attention_mask, position_bias, encoder_hidden_states, past_key_values) -> bool:
        from transformers.activations import NewGELUActivation
        from transformers.models.t5.modeling_t5 import T5DenseGatedActDense

        att, dense = self.layer[0].SelfAttention, self.layer[-1].DenseReluDense
        if not (hidden_states.is_cuda and hidden_states.dim() == 3 and hidden_states.dtype in (torch.bfloat16, torch.float16)
                and not self.is_decoder and not self.training and encoder_hidden_states is None and past_key_values is None
                and not (torch.is_grad_enabled() and hidden_states.requires_grad)
                and att.key_value_proj_dim == 64 and hidden_states.shape[-1] % 8 == 0
                and isinstance(dense, T5DenseGatedActDense) and isinstance(dense.act, NewGELUActivation)):
            return False
        linears = (att.q, att.k, att.v, att.o, dense.wi_0, dense.wi_1, dense.wo)
        if not all(isinstance(m, W4Linear) and m.group_size == 128 and m.scales.dtype == hidden_states.dtype for m in linears):
            return False
        B, T, _ = hidden_states.shape
        if position_bias is not None and not (isinstance(position_bias, torch.Tensor) and tuple(position_bias.shape) == (1, att.n_heads, T, T)):
            return False
        return _key_bias(attention_mask, B, T)[0]

    def forward(self, hidden_states, attention_mask=None, position_bias=None, encoder_hidden_states=None, encoder_attention_mask=None,
                encoder_decoder_position_bias=None, past_key_values=None, **kwargs):
        handed, self._handed = self._handed, None
        if not self._serves(hidden_states, attention_mask, position_bias, encoder_hidden_states, past_key_values):
            return super().forward(hidden_states, attention_mask, position_bias, encoder_hidden_states, encoder_attention_mask,
                                   encoder_decoder_position_bias, past_key_values=past_key_values, **kwargs)
        from ...ops.attention import attention_d64_bias
        from ...ops.elementwise import t5_residual_norm
        from ...ops.gemm import gemm_awq_multi

        sa, ff = self.layer[0], self.layer[-1]
        att, dense = sa.SelfAttention, ff.DenseReluDense
        B, T, _ = hidden_states.shape
        H, inner = att.n_heads, att.n_heads * 64
        fp16 = hidden_states.dtype == torch.float16
        if handed is not None and handed[0] is hidden_states:
            normed = handed[1]
        else:
            normed = t5_residual_norm(hidden_states, None, sa.layer_norm.weight.data, sa.layer_norm.variance_epsilon)[1]
        qkv = gemm_awq_multi(normed, (att.q, att.k, att.v), "concat")
        if position_bias is None:  # (T5Attention.forward: the first layer computes it, the stack shares it)
            if att.has_relative_attention_bias:
                position_bias = att.compute_bias(T, T, device=hidden_states.device, past_seen_tokens=0)
            else:
                position_bias = torch.zeros((1, H, T, T), device=hidden_states.device, dtype=hidden_states.dtype)
        ctx = attention_d64_bias(qkv[..., :inner], qkv[..., inner:2 * inner], qkv[..., 2 * inner:], H, toeplitz_rel_bias(position_bias),
                                 _key_bias(attention_mask, B, T)[1], scale=1.0 if att.scaling is None else att.scaling)
        o = att.o(ctx)
        w_ff, eps_ff = ff.layer_norm.weight.data, ff.layer_norm.variance_epsilon
        if fp16:
            y = self._clamp(t5_residual_norm(hidden_states, o)[0])
            n2 = t5_residual_norm(y, None, w_ff, eps_ff)[1]
        else:
            y, n2, _ = t5_residual_norm(hidden_states, o, w_ff, eps_ff)
        f = dense.wo(gemm_awq_multi(n2, (dense.wi_0, dense.wi_1), "gated_gelu_new"))
        nxt = self._next
        if fp16 or nxt is None:
            out = t5_residual_norm(y, f)[0]
            if fp16:
                out = self._clamp(out)
        else:
            norm = nxt.layer[0].layer_norm
            out, n_next, _ = t5_residual_norm(y, f, norm.weight.data, norm.variance_epsilon)
            nxt._handed = (out, n_next)
        return out, position_bias, None

    @staticmethod
    def _clamp(hidden_states):
        """T5Block.forward's "clamp inf values" step, the same torch operations"""
        clamp_value = torch.where(torch.isinf(hidden_states).any(), torch.finfo(hidden_states.dtype).max - 1000, torch.finfo(hidden_states.dtype).max)
        return torch.clamp(hidden_states, min=-clamp_value, max=clamp_value)


def set_fused_layers(model, enabled: bool = True):
    """Swap the classes of ``model.encoder``'s blocks and final norm between transformers' and the fused ones (:class:`FusedT5Block`,
    :class:`FusedT5LayerNorm`).  Modules, parameters, buffers and ``state_dict()`` keys are untouched; off restores the parent's path exactly."""
    blocks = list(model.encoder.block)
    for i, blk in enumerate(blocks):
        if enabled and type(blk) is T5Block:
            blk.__class__ = FusedT5Block
        elif not enabled and type(blk) is FusedT5Block:
            blk.__class__ = T5Block
        blk.__dict__.pop("_next", None)
        blk.__dict__.pop("_handed", None)
    if enabled:
        for blk, nxt in zip(blocks, blocks[1:]):
            if type(blk) is FusedT5Block and type(nxt) is FusedT5Block:
                object.__setattr__(blk, "_next", nxt)
    norm = model.encoder.final_layer_norm
    if enabled and type(norm) is T5LayerNorm:
        norm.__class__ = FusedT5LayerNorm
    elif not enabled and type(norm) is FusedT5LayerNorm:
        norm.__class__ = T5LayerNorm
    return model


class NunchakuT5EncoderModel(T5EncoderModel):
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str | os.PathLike, **kwargs) -> T5EncoderModel:
        """``pretrained_model_name_or_path``: a local ``.safetensors`` file whose metadata entry ``config`` holds the T5 config
        as JSON (hub names are not resolved).  ``torch_dtype`` (default bfloat16) is the compute dtype, ``device`` (default
        ``"cuda"``) where the model is materialised.  The model is built on the meta device, its quantised linears swapped
        for W4Linear (group 128), then materialised and loaded with ``strict=True``.  ``fused_attention`` (default True) selects
        :func:`fused_t5_attention` on the model's config when the device is a GPU, ``d_kv == 64`` and the model is an encoder; False keeps
        transformers' eager attention.  ``fused_layers`` (default False) puts the encoder's layers on the fused kernels
        (:func:`set_fused_layers`: q / k / v and the gated-GELU feed-forward as one ``gemm_awq_multi`` launch each, residual adds and norms as
        ``t5_residual_norm`` passes); the returned model has ``set_fused_layers(bool)`` to switch at any time."""
        path = os.fspath(pretrained_model_name_or_path)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"NunchakuT5EncoderModel.from_pretrained: {path!r} is not a local .safetensors file "
                                    "(download the checkpoint first; hub names are not resolved)")
        state_dict, meta = _read_safetensors(path)
        if "config" not in meta:
            raise ValueError(f"{path}: no 'config' entry in the safetensors metadata")
        config = T5Config(**json.loads(meta["config"]))
        dtype = kwargs.get("torch_dtype", torch.bfloat16)
        with torch.device("meta"):
            model = T5EncoderModel(config).to(dtype)
        model.eval()
        modules = dict(model.named_modules())
        for name, module in list(modules.items()):
            if isinstance(module, nn.Linear) and f"{name}.qweight" in state_dict:
                q = W4Linear.from_linear(module, group_size=128, init_only=True)
                parent, child = name.rsplit(".", 1)
                setattr(modules[parent], child, q)
        for a, b in (_TIED, _TIED[::-1]):
            if a not in state_dict and b in state_dict:
                state_dict[a] = state_dict[b]
        device = torch.device(kwargs.get("device", "cuda"))
        model.to_empty(device=device)
        model.load_state_dict(state_dict, strict=True)
        if (kwargs.get("fused_attention", True) and device.type == "cuda" and config.d_kv == 64 and not config.is_decoder
                and register_fused_attention()):
            model.config._attn_implementation = ATTENTION_NAME
        model.__class__ = cls  # (T5EncoderModel plus set_fused_layers: no other attribute or method differs)
        if kwargs.get("fused_layers", False):
            set_fused_layers(model, True)
        return model

    def set_fused_layers(self, enabled: bool = True):
        """see :func:`set_fused_layers`"""
        return set_fused_layers(self, enabled)
