"""SANA: the linear-attention layer, the cross-attention, the feed-forward, the transformer block and the stack of blocks (reference:
src/SanaModel.cpp:13-136 ``SanaLinearAttention``, :138-190 ``MultiHeadCrossAttention``, :192-213 ``SanaGLUMBConv``, :215-322
``SanaLinearTransformerBlock``, :324-363 ``SanaModel``).

The attention: the QKV projection, ReLU linear attention over its packed output
(``svdq_linear_attention``: a kernel of its own, where the reference folds the K/V reduction into the GEMM's epilogue with atomics) and the
output projection.  The feed-forward (GLU-MBConv): a GEMM with a SiLU epilogue, a depthwise 3x3 convolution over the token grid
(``svdq_dwconv3x3``: a kernel of its own, where the reference instantiates a CUTLASS template) and a GEMM whose quantiser applies the GLU.
The cross-attention: a W4A4 query projection, a 16-bit K/V projection of the text condition, attention over per-sample key ranges
(``svdq_cross_attention``: a kernel of its own, where the reference calls flash-attention's ``mha_varlen_fwd``) and a W4A4 output projection.
The block: the three layers around a residual stream with the element-wise glue between them -- gated residual, LayerNorm, the next layer's
per-sample modulation and the padding to the GEMM operand width -- in one row pass (``svdq_sana_glue``: a kernel of its own, three launches per
block where the reference runs nine); :class:`SanaModel` chains the blocks so that the pass behind a feed-forward already modulates the next
block's input.  The diffusers-facing class ``NunchakuSanaTransformer2DModel`` is in ``transformer_sana.py``.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from ..ops.attention import CROSS_ATTENTION_MAX_KEYS, cross_attention, linear_attention
from ..ops.conv import dwconv3x3, grid_of
from ..ops.elementwise import SANA_MLP, SANA_MSA, sana_glue
from .linear import SVDQW4A4Linear

HEAD_DIM = 32


class SanaLinearAttention(nn.Module):
    """``out_proj(linear_attention(qkv_proj(x)))`` with 32-channel heads.

    Sub-modules carry the reference's names (SanaModel.cpp:17-22): ``qkv_proj`` [dim_pad -> 3 * dim_pad], ``out_proj`` [dim_pad -> dim_pad] and,
    with ``pag``, ``pag_to_v`` [dim_pad -> dim_pad], where ``dim_pad = ceil(dim / 128) * 128``: the reference's 4-bit GEMM pads both feature
    counts to 128 (src/Linear.cpp:92-107), so a checkpoint's tensors already have the padded shapes (SANA-1.6B: 2240 -> 2304, 72 heads).
    Legacy key names are mapped by :func:`convert_sana_attention_state_dict`; the result loads with ``strict=True``.

    Tokens are NOT padded per batch element: the kernel takes ``T``.  The reference pads every batch element to 256 tokens with zero rows
    and sums over them, so with ``bias=True`` those rows would add ``relu(bias_k)`` and ``bias_v * relu(bias_k)`` to its ``vk``; here they do
    not exist.  SANA's attention has ``bias=False``, where the two agree."""

    def __init__(self, dim: int, bias: bool = False, pag: bool = False, rank: int = 32, torch_dtype: torch.dtype = torch.bfloat16,
                 device: str | torch.device | None = None):
        super().__init__()
        self.dim = dim
        self.dim_pad = (dim + 127) // 128 * 128
        self.heads = self.dim_pad // HEAD_DIM
        kw = dict(rank=rank, bias=bias, torch_dtype=torch_dtype, device=device)
        self.qkv_proj = SVDQW4A4Linear(self.dim_pad, 3 * self.dim_pad, **kw)
        self.out_proj = SVDQW4A4Linear(self.dim_pad, self.dim_pad, **kw)
        self.pag_to_v = SVDQW4A4Linear(self.dim_pad, self.dim_pad, **kw) if pag else None

    def _padded(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 3 or x.shape[-1] not in (self.dim, self.dim_pad):
            raise ValueError(f"SanaLinearAttention: expected x [B, T, {self.dim}], got {tuple(x.shape)}")
        # (a [B, T, dim_pad] input is the transformer block's: already padded, zeros behind column dim)
        return x if x.shape[-1] == self.dim_pad else F.pad(x, (0, self.dim_pad - self.dim))

    @staticmethod
    def _deliver(y: torch.Tensor, out: torch.Tensor | None) -> torch.Tensor:
        if out is None:
            return y
        out.copy_(y)
        return out

    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """x [B, T, dim] -> [B, T, dim] (into ``out`` when given)"""
        qkv = self.qkv_proj(self._padded(x))            # [B, T, 3 * dim_pad]: Q, then (K, V) per head
        attn = linear_attention(qkv, self.heads)        # [B, T, dim_pad], token-major
        return self._deliver(self.out_proj(attn)[..., : self.dim], out)

    def forward_pag(self, x: torch.Tensor, cfg: bool) -> torch.Tensor:
        """Perturbed-attention guidance (SanaModel.cpp:108-136): the first 2/3 (``cfg``) or the first half of the batch goes through
        :meth:`forward`, the rest -- the perturbed samples, whose attention is the identity -- through ``out_proj(pag_to_v(x))``."""
        if self.pag_to_v is None:
            raise RuntimeError("SanaLinearAttention.forward_pag: the layer was built without pag_to_v (pag=False)")
        B = x.shape[0]
        parts = 3 if cfg else 2
        if B % parts:
            raise ValueError(f"SanaLinearAttention.forward_pag: batch size {B} is not a multiple of {parts} (cfg={bool(cfg)})")
        n = B * (parts - 1) // parts
        out = torch.empty(B, x.shape[1], self.dim, dtype=x.dtype, device=x.device)
        x = self._padded(x)
        self.forward(x[:n], out[:n])
        self._deliver(self.out_proj(self.pag_to_v(self._padded(x[n:])))[..., : self.dim], out[n:])
        return out


class SanaDepthwiseConv(nn.Module):
    """The reference's ``DWCONV`` (src/Linear.cpp:542-551): ``weight`` [C, 3, 3, 1] and ``bias`` [C] in the activation dtype, a depthwise 3x3
    cross-correlation with zero padding 1 over a channels-last ``[B, H, W, C]`` activation (``ops.conv.dwconv3x3``)."""

    def __init__(self, channels: int, bias: bool = True, torch_dtype: torch.dtype = torch.bfloat16, device: str | torch.device | None = None):
        super().__init__()
        self.channels = channels
        self.weight = nn.Parameter(torch.empty(channels, 3, 3, 1, dtype=torch_dtype, device=device), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(channels, dtype=torch_dtype, device=device), requires_grad=False) if bias else None

    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """x [B, H, W, C] -> [B, H, W, C] (into ``out`` when given: it may be a column slice of a wider buffer)"""
        return dwconv3x3(x, self.weight, self.bias, out=out)


def _ceil128(n: int) -> int:
    return (n + 127) // 128 * 128


class SanaGLUMBConv(nn.Module):
    """``point_conv(glu(depth_conv(silu(inverted_conv(x)))))`` over a grid of ``H x W`` tokens (SanaModel.cpp:192-213).

    Sub-modules carry the reference's names (SanaModel.cpp:195-198): ``inverted_conv`` [in_pad -> C_gemm] with bias, ``depth_conv``
    (``weight`` [C_gemm, 3, 3, 1], ``bias`` [C_gemm]) and ``point_conv`` [hid_pad -> in_pad] without bias, where ``in_pad = ceil128(in_features)``,
    ``C_gemm = ceil128(2 * hidden_features)`` and ``hid_pad = ceil128(hidden_features)``: the reference's 4-bit GEMM pads both of its feature
    counts to 128 (src/Linear.cpp:92-107), and the convolution runs on what the first GEMM wrote, so its parameters have that width too
    (a ``depth_conv`` tensor of ``2 * hidden_features`` channels is padded with zeros behind its last channel before it is loaded).
    SANA-1.6B: (2240, 5600) -> (2304, 11264, 5632); SANA-0.6B: (1152, 2880) -> (1152, 5760, 2944).

    ``point_conv``'s quantiser reads ``2 * hid_pad`` interleaved (value, gate) columns, which is ``C_gemm`` for the first and 128 more than
    ``C_gemm`` for the second: the convolution writes its ``C_gemm`` channels into a buffer ``2 * hid_pad`` wide whose tail columns are zeroed
    where it is allocated -- ``0 * silu(0) = 0``, so the padded input channels of ``point_conv`` see zeros.
    Legacy key names are mapped by :func:`convert_sana_ff_state_dict`; the result loads with ``strict=True``."""

    def __init__(self, in_features: int, hidden_features: int, rank: int = 32, torch_dtype: torch.dtype = torch.bfloat16,
                 device: str | torch.device | None = None):
        super().__init__()
        self.in_features, self.hidden_features = in_features, hidden_features
        self.in_pad, self.c_gemm, self.hid_pad = _ceil128(in_features), _ceil128(2 * hidden_features), _ceil128(hidden_features)
        kw = dict(rank=rank, torch_dtype=torch_dtype, device=device)
        self.inverted_conv = SVDQW4A4Linear(self.in_pad, self.c_gemm, bias=True, **kw)
        self.depth_conv = SanaDepthwiseConv(self.c_gemm, bias=True, torch_dtype=torch_dtype, device=device)
        self.point_conv = SVDQW4A4Linear(self.hid_pad, self.in_pad, bias=False, **kw)

    def gated_input(self, x: torch.Tensor, H: int | None = None, W: int | None = None) -> torch.Tensor:
        """x [B, T, in_features] -> the [B, T, 2 * hid_pad] (value, gate) buffer ``point_conv``'s quantiser reads: ``depth_conv(silu(inverted_conv(x)))``
        in its first ``C_gemm`` columns, zeros behind them."""
        if x.dim() != 3 or x.shape[-1] not in (self.in_features, self.in_pad):
            raise ValueError(f"SanaGLUMBConv: expected x [B, T, {self.in_features}], got {tuple(x.shape)}")
        B, T = x.shape[:2]
        H, W = grid_of(T, H, W)
        if x.shape[-1] != self.in_pad:                                       # (in_pad wide: the transformer block's, zeros behind column in_features)
            x = F.pad(x, (0, self.in_pad - self.in_features))
        y = self.inverted_conv.forward_silu(x)                               # [B, T, C_gemm]: one GEMM launch, SiLU in its epilogue
        wide = torch.empty(B, T, 2 * self.hid_pad, dtype=y.dtype, device=y.device)
        if 2 * self.hid_pad != self.c_gemm:
            wide[..., self.c_gemm:].zero_()                                  # (the tail of THIS allocation; the convolution never writes it)
        self.depth_conv(y.unflatten(1, (H, W)), out=wide[..., : self.c_gemm].unflatten(1, (H, W)))
        return wide

    def forward(self, x: torch.Tensor, H: int | None = None, W: int | None = None) -> torch.Tensor:
        """x [B, T, in_features] on a grid of ``H x W = T`` tokens (without the pair: a square grid; one missing side is derived) -> [B, T, in_features]"""
        wide = self.gated_input(x, H, W)
        B, T = wide.shape[:2]
        qx, ascales, lora_act = self.point_conv.quantize(wide.view(B * T, -1), fuse_glu=True)
        out = torch.empty(B * T, self.in_pad, dtype=wide.dtype, device=wide.device)
        return self.point_conv.forward_quant(qx, ascales, lora_act, out).view(B, T, -1)[..., : self.in_features]


class SanaCrossAttention(nn.Module):
    """``out_proj(cross_attention(q_linear(x), kv_linear(cond)))`` over per-sample ranges of text tokens (SanaModel.cpp:138-190).

    Sub-modules carry the reference's names (SanaModel.cpp:141-144): ``q_linear`` and ``out_proj`` are W4A4 [dim_pad -> dim_pad] with bias, where
    ``dim = num_heads * head_dim`` and ``dim_pad = ceil128(dim)`` (the reference's 4-bit GEMM pads both feature counts to 128, src/Linear.cpp:92-107;
    SANA-1.6B: 20 x 112 = 2240 -> 2304, SANA-0.6B: 16 x 72 = 1152); ``kv_linear`` is an ``nn.Linear(dim, 2 * dim)`` in the activation dtype (the
    reference's ``GEMM_F16``, not padded): K in its first ``dim`` output columns, V in the rest.  ``head_dim`` 72, 112 or 128.
    Legacy key names are mapped by :func:`convert_sana_cross_attention_state_dict`; the result loads with ``strict=True``.

    The attention reads Q in place from the first ``dim`` columns of ``q_linear``'s ``dim_pad``-wide rows and K / V in place from the two column
    halves of ``kv_linear``'s output, and writes into the first ``dim`` columns of a ``dim_pad``-wide buffer whose tail is zeroed where it is
    allocated: ``out_proj``'s padded input channels see zeros.  A sample has at most 320 text tokens (``max_sequence_length`` is 300).
    K and V of a condition are computed on every call; they do not change over the denoising steps, so the model class can cache them."""

    def __init__(self, num_heads: int, head_dim: int, rank: int = 32, torch_dtype: torch.dtype = torch.bfloat16,
                 device: str | torch.device | None = None):
        super().__init__()
        if head_dim not in (72, 112, 128):
            raise ValueError(f"SanaCrossAttention: head_dim={head_dim}: the cross-attention kernel has 72, 112 and 128")
        self.num_heads, self.head_dim = num_heads, head_dim
        self.dim = num_heads * head_dim
        self.dim_pad = _ceil128(self.dim)
        kw = dict(rank=rank, bias=True, torch_dtype=torch_dtype, device=device)
        self.q_linear = SVDQW4A4Linear(self.dim_pad, self.dim_pad, **kw)
        self.kv_linear = nn.Linear(self.dim, 2 * self.dim, bias=True, dtype=torch_dtype, device=device)
        self.kv_linear.requires_grad_(False)
        self.out_proj = SVDQW4A4Linear(self.dim_pad, self.dim_pad, **kw)

    def _attend(self, x: torch.Tensor, cond2: torch.Tensor, max_keys: int, **ranges) -> torch.Tensor:
        B, T = x.shape[:2]
        if x.shape[-1] != self.dim_pad:                                      # (dim_pad wide: the transformer block's, zeros behind column dim)
            x = F.pad(x, (0, self.dim_pad - self.dim))
        q = self.q_linear(x)                                                 # [B, T, dim_pad]; the first dim columns are Q
        kv = self.kv_linear(cond2)                                           # [Ntxt, 2 * dim]: K | V
        wide = torch.empty(B, T, self.dim_pad, dtype=q.dtype, device=q.device)
        if self.dim_pad != self.dim:
            wide[..., self.dim:].zero_()                                     # (the tail of THIS allocation; the attention never writes it)
        cross_attention(q, kv[:, : self.dim], kv[:, self.dim:], self.num_heads, self.head_dim, max_keys=max_keys, out=wide[..., : self.dim], **ranges)
        return self.out_proj(wide)[..., : self.dim]

    def _check_x(self, x: torch.Tensor):
        if x.dim() != 3 or x.shape[-1] not in (self.dim, self.dim_pad):
            raise ValueError(f"SanaCrossAttention: expected x [B, T, {self.dim}], got {tuple(x.shape)}")

    def forward(self, x: torch.Tensor, cond: torch.Tensor, cu_seqlens_img: torch.Tensor | None, cu_seqlens_txt: torch.Tensor) -> torch.Tensor:
        """x [B, T, dim], cond [Ntxt, dim] (the samples' text tokens, packed), cu_seqlens_txt int32 [B + 1] on the device -> [B, T, dim].
        ``cu_seqlens_img`` may be None and is otherwise checked for its length only: every sample has T image tokens (the reference's Python
        always builds it uniform).  A sample may hold at most 320 text tokens: the ranges are not read on the host, the kernel is given
        ``max_keys = min(Ntxt, 320)`` and a longer sample is cut to its first 320 tokens WITHOUT an error (:meth:`forward_padded` refuses ``L > 320``)."""
        self._check_x(x)
        B = x.shape[0]
        if cond.dim() != 2 or cond.shape[-1] != self.dim:
            raise ValueError(f"SanaCrossAttention: expected cond [Ntxt, {self.dim}], got {tuple(cond.shape)}")
        if cu_seqlens_txt is None or cu_seqlens_txt.dim() != 1 or cu_seqlens_txt.shape[0] != B + 1:
            raise ValueError(f"SanaCrossAttention: cu_seqlens_txt must be [B + 1] = [{B + 1}], got {None if cu_seqlens_txt is None else tuple(cu_seqlens_txt.shape)}")
        if cu_seqlens_img is not None and (cu_seqlens_img.dim() != 1 or cu_seqlens_img.shape[0] != B + 1):
            raise ValueError(f"SanaCrossAttention: cu_seqlens_img must be [B + 1] = [{B + 1}] or None, got {tuple(cu_seqlens_img.shape)}")
        return self._attend(x, cond, min(cond.shape[0], CROSS_ATTENTION_MAX_KEYS), cu_seqlens=cu_seqlens_txt)

    def forward_padded(self, x: torch.Tensor, cond: torch.Tensor, key_counts: torch.Tensor) -> torch.Tensor:
        """x [B, T, dim], cond [B, L, dim] (every sample's text tokens first, padding behind them), key_counts int32 [B] on the device
        (``mask.sum(1)``) -> [B, T, dim].  No boolean index, no host synchronisation: the call can be captured."""
        self._check_x(x)
        B = x.shape[0]
        if cond.dim() != 3 or cond.shape[0] != B or cond.shape[-1] != self.dim:
            raise ValueError(f"SanaCrossAttention: expected cond [{B}, L, {self.dim}], got {tuple(cond.shape)}")
        L = cond.shape[1]
        if L > CROSS_ATTENTION_MAX_KEYS:
            raise ValueError(f"SanaCrossAttention: L={L} text tokens per sample: at most {CROSS_ATTENTION_MAX_KEYS}")
        if key_counts is None or tuple(key_counts.shape) != (B,):
            raise ValueError(f"SanaCrossAttention: key_counts must be [B] = [{B}], got {None if key_counts is None else tuple(key_counts.shape)}")
        offsets = torch.arange(0, B * L, L, dtype=torch.int32, device=x.device) if L > 0 else torch.zeros(B, dtype=torch.int32, device=x.device)
        return self._attend(x, cond.reshape(B * L, self.dim), L, key_offsets=offsets, key_counts=key_counts)


def convert_sana_attention_state_dict(sd: dict) -> dict:
    """Legacy parameter names -> this project's (what the reference's FLUX converter does, transformer_flux_v2.py:591-596, 623-628):
    ``lora_down`` -> ``proj_down``, ``lora_up`` -> ``proj_up``, ``smooth`` -> ``smooth_factor``, ``smooth_orig`` -> ``smooth_factor_orig``.
    Keys that already carry the new names pass through."""
    new = {}
    for k, v in sd.items():
        nk = k.replace(".lora_down", ".proj_down").replace(".lora_up", ".proj_up")
        if ".smooth_factor" not in k:
            if ".smooth_orig" in k:
                nk = nk.replace(".smooth_orig", ".smooth_factor_orig")
            elif ".smooth" in k:
                nk = nk.replace(".smooth", ".smooth_factor")
        new[nk] = v
    return new


def convert_sana_ff_state_dict(sd: dict) -> dict:
    """The same mapping for the keys of one ``ff`` block (``inverted_conv.*``, ``point_conv.*``); ``depth_conv.weight`` and ``depth_conv.bias`` carry
    none of the legacy names and pass through."""
    return convert_sana_attention_state_dict(sd)


def convert_sana_cross_attention_state_dict(sd: dict) -> dict:
    """The same mapping for the keys of one ``cross_attn`` block (``q_linear.*``, ``out_proj.*``); ``kv_linear.weight`` and ``kv_linear.bias`` carry
    none of the legacy names and pass through."""
    return convert_sana_attention_state_dict(sd)


class SanaLinearTransformerBlock(nn.Module):
    """One SANA block (reference: ``SanaLinearTransformerBlock``, src/SanaModel.cpp:215-322): linear attention, cross-attention and GLU-MBConv
    around a residual stream, modulated per sample by ``timestep [B, 6, dim] + scale_shift_table [6, dim]`` (rows: shift / scale / gate of the
    attention, then of the feed-forward).  Children ``attn``, ``cross_attn``, ``ff`` and the parameter ``scale_shift_table`` carry the reference's
    names; its two LayerNorms have no parameters (``elementwise_affine=False``, eps 1e-6) and live inside the glue kernel here.

    The element-wise glue is ``ops.elementwise.sana_glue`` (``svdq_sana_glue``), three launches per block where the reference has nine:
    gate_msa + residual; the cross-attention residual with the feed-forward's modulated LayerNorm; gate_mlp + residual with the NEXT block's
    attention-modulated LayerNorm (the stack passes that block's table; :meth:`forward` on its own computes its first modulation itself: one
    launch more).  The block keeps the residual stream and the modulated inputs ``dim_pad = ceil128(dim)`` wide with a zero tail, the width of
    the 4-bit GEMMs' operands, so the three layers pad nothing."""

    def __init__(self, hidden_size: int, intermediate_size: int, num_cross_attention_heads: int, pag: bool = False, rank: int = 32,
                 torch_dtype: torch.dtype = torch.bfloat16, device: str | torch.device | None = None):
        super().__init__()
        if hidden_size % num_cross_attention_heads:
            raise ValueError(f"SanaLinearTransformerBlock: hidden_size={hidden_size} is not a multiple of num_cross_attention_heads={num_cross_attention_heads}")
        self.hidden_size, self.intermediate_size, self.num_cross_attention_heads = hidden_size, intermediate_size, num_cross_attention_heads
        self.dim_pad = _ceil128(hidden_size)
        kw = dict(rank=rank, torch_dtype=torch_dtype, device=device)
        self.attn = SanaLinearAttention(hidden_size, bias=False, pag=pag, **kw)
        self.cross_attn = SanaCrossAttention(num_cross_attention_heads, hidden_size // num_cross_attention_heads, **kw)
        self.ff = SanaGLUMBConv(hidden_size, intermediate_size, **kw)
        self.scale_shift_table = nn.Parameter(torch.empty(6, hidden_size, dtype=torch_dtype, device=device), requires_grad=False)

    # ---- the glue -------------------------------------------------------------------------------------------------------------------------
    def _timestep3(self, hidden_states: torch.Tensor, timestep: torch.Tensor) -> torch.Tensor:
        B, dim = hidden_states.shape[0], self.hidden_size
        if hidden_states.dim() != 3 or hidden_states.shape[-1] not in (dim, self.dim_pad):
            raise ValueError(f"SanaLinearTransformerBlock: expected hidden_states [B, T, {dim}], got {tuple(hidden_states.shape)}")
        if timestep is None or timestep.numel() != B * 6 * dim or timestep.shape[0] != B:
            raise ValueError(f"SanaLinearTransformerBlock: timestep must be [B, 6 * dim] = [{B}, {6 * dim}], got {None if timestep is None else tuple(timestep.shape)}")
        return timestep.to(hidden_states.dtype).reshape(B, 6, dim)

    def modulate_msa(self, hidden_states: torch.Tensor, timestep3: torch.Tensor):
        """``(residual stream [B, T, dim_pad], attention input [B, T, dim_pad])`` of this block for a ``hidden_states`` that no glue pass of a
        block before it has modulated: one launch.  The stream is ``hidden_states`` itself when it needs no padding."""
        wide = hidden_states.shape[-1] == self.dim_pad
        h, hm, _ = sana_glue(hidden_states, None, timestep=timestep3, mod_table=self.scale_shift_table, scale_row=SANA_MSA[1], shift_row=SANA_MSA[0],
                             channels=self.hidden_size, pad_to=self.dim_pad, out=not wide, out_mod=True)
        return (hidden_states if wide else h), hm

    def _core(self, h: torch.Tensor, hm: torch.Tensor, cross, timestep3: torch.Tensor, H, W, pag: bool, cfg: bool, next_table: torch.Tensor | None,
              own_stream: bool):
        """h, hm: the ``dim_pad``-wide residual stream and attention input; ``cross``: ``x -> cross-attention output``; ``next_table``: the
        ``scale_shift_table`` of the block that follows (None: nothing follows); ``own_stream``: ``h`` may be overwritten.
        Returns ``(stream, the next block's attention input or None)``."""
        glue = dict(timestep=timestep3, channels=self.hidden_size, pad_to=self.dim_pad)
        tab = self.scale_shift_table
        a = self.attn.forward_pag(hm, cfg) if pag else self.attn(hm)
        h, _, _ = sana_glue(h, a, gate_table=tab, gate_row=SANA_MSA[2], out=h if own_stream else True, out_mod=False, **glue)
        a = cross(h)
        h, hm, _ = sana_glue(h, a, mod_table=tab, scale_row=SANA_MLP[1], shift_row=SANA_MLP[0], out=h, out_mod=True, **glue)
        a = self.ff(hm, H, W)
        if next_table is None:
            h, _, _ = sana_glue(h, a, gate_table=tab, gate_row=SANA_MLP[2], out=h, out_mod=False, **glue)
            return h, None
        h, hm, _ = sana_glue(h, a, gate_table=tab, gate_row=SANA_MLP[2], mod_table=next_table, scale_row=SANA_MSA[1], shift_row=SANA_MSA[0],
                             out=h, out_mod=True, **glue)
        return h, hm

    def _cross_packed(self, cond, cu_seqlens_img, cu_seqlens_txt):
        return lambda x: self.cross_attn(x, cond, cu_seqlens_img, cu_seqlens_txt)

    def _cross_padded(self, cond, key_counts):
        return lambda x: self.cross_attn.forward_padded(x, cond, key_counts)

    def _alone(self, hidden_states, timestep, cross, H, W, pag, cfg):
        t3 = self._timestep3(hidden_states, timestep)
        h, hm = self.modulate_msa(hidden_states, t3)
        h, _ = self._core(h, hm, cross, t3, H, W, pag, cfg, None, own_stream=h is not hidden_states)
        return h[..., : self.hidden_size]

    def forward(self, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor, timestep: torch.Tensor, cu_seqlens_img: torch.Tensor | None,
                cu_seqlens_txt: torch.Tensor, H: int | None = None, W: int | None = None, pag: bool = False, cfg: bool = False) -> torch.Tensor:
        """The reference's argument list (SanaModel.cpp:234-242): hidden_states [B, T, dim], encoder_hidden_states [Ntxt, dim] (the samples' text
        tokens, packed), timestep [B, 6 * dim], cu_seqlens_txt int32 [B + 1] on the device, a grid of ``H x W = T`` tokens -> [B, T, dim]."""
        return self._alone(hidden_states, timestep, self._cross_packed(encoder_hidden_states, cu_seqlens_img, cu_seqlens_txt), H, W, pag, cfg)

    def forward_padded(self, hidden_states: torch.Tensor, cond: torch.Tensor, timestep: torch.Tensor, key_counts: torch.Tensor,
                       H: int | None = None, W: int | None = None, pag: bool = False, cfg: bool = False) -> torch.Tensor:
        """:meth:`forward` on a padded condition: cond [B, L, dim] (every sample's text tokens first), key_counts int32 [B] on the device
        (``SanaCrossAttention.forward_padded``).  No boolean index, no host synchronisation: the call can be captured."""
        return self._alone(hidden_states, timestep, self._cross_padded(cond, key_counts), H, W, pag, cfg)


def sana_intermediate_size(inner_dim: int, mlp_ratio: float) -> int:
    """``ceil(round(mlp_ratio * inner_dim) / 64) * 64`` (SanaModel.cpp:329).  At the ratio 2.5: 1152 -> 2880; 2240 -> round gives 5600, the
    next multiple of 64 is 5632 -- the feed-forward's GEMM operands are those of 5600 (``ceil128(5600) = 5632``, ``ceil128(11200) = 11264``)."""
    return (int(round(mlp_ratio * inner_dim)) + 63) // 64 * 64


def _config_get(config, key: str, default=None):
    if isinstance(config, dict) or hasattr(config, "keys"):
        return config[key] if key in config else default
    return getattr(config, key, default)


class SanaModel(nn.Module):
    """The stack of blocks (reference: ``SanaModel`` / ``QuantizedSanaModel``, src/SanaModel.cpp:324-363, nunchaku/csrc/sana.h): ``config`` gives
    ``num_layers``, ``num_attention_heads``, ``attention_head_dim``, ``num_cross_attention_heads`` and ``mlp_ratio`` (a dict, or an object with
    these attributes); ``pag_layers``: the layers built with ``pag_to_v`` -- perturbed-attention guidance applies on these only.

    :meth:`forward` issues the first block's attention modulation itself (one glue launch) and hands every block the table of the block behind
    it, so the pass behind a feed-forward also modulates the next block's input: 3 glue launches per block plus 1 per forward.
    :meth:`forward_layer` is self-contained (4 launches)."""

    def __init__(self, config, pag_layers=(), torch_dtype: torch.dtype = torch.bfloat16, device: str | torch.device | None = None, rank: int = 32):
        super().__init__()
        heads, head_dim = int(_config_get(config, "num_attention_heads")), int(_config_get(config, "attention_head_dim"))
        self.num_layers = int(_config_get(config, "num_layers"))
        self.inner_dim = heads * head_dim
        self.intermediate_size = sana_intermediate_size(self.inner_dim, float(_config_get(config, "mlp_ratio", 2.5)))
        pag_layers = [pag_layers] if isinstance(pag_layers, int) else list(pag_layers or ())
        if any(not 0 <= i < self.num_layers for i in pag_layers):
            raise ValueError(f"SanaModel: pag_layers={pag_layers} outside the {self.num_layers} layers")
        self.pag_layers = sorted(set(pag_layers))
        self.transformer_blocks = nn.ModuleList(
            SanaLinearTransformerBlock(self.inner_dim, self.intermediate_size, int(_config_get(config, "num_cross_attention_heads")),
                                       pag=i in self.pag_layers, rank=rank, torch_dtype=torch_dtype, device=device) for i in range(self.num_layers))

    def _run(self, hidden_states, timestep, make_cross, H, W, pag, cfg, skip_first_layer):
        first = 1 if skip_first_layer else 0
        blocks = self.transformer_blocks
        if first >= len(blocks):
            return hidden_states
        t3 = blocks[first]._timestep3(hidden_states, timestep)
        h, hm = blocks[first].modulate_msa(hidden_states, t3)
        own = h is not hidden_states
        for i in range(first, len(blocks)):
            nxt = blocks[i + 1].scale_shift_table if i + 1 < len(blocks) else None
            h, hm = blocks[i]._core(h, hm, make_cross(blocks[i]), t3, H, W, bool(pag) and i in self.pag_layers, cfg, nxt, own_stream=own)
            own = True
        return h[..., : self.inner_dim]

    def forward(self, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor, timestep: torch.Tensor, cu_seqlens_img: torch.Tensor | None,
                cu_seqlens_txt: torch.Tensor, H: int | None = None, W: int | None = None, pag: bool = False, cfg: bool = False,
                skip_first_layer: bool = False) -> torch.Tensor:
        """The reference's argument list (SanaModel.cpp:339-348); see :meth:`SanaLinearTransformerBlock.forward`."""
        return self._run(hidden_states, timestep, lambda b: b._cross_packed(encoder_hidden_states, cu_seqlens_img, cu_seqlens_txt), H, W, pag, cfg,
                         skip_first_layer)

    def forward_padded(self, hidden_states: torch.Tensor, cond: torch.Tensor, timestep: torch.Tensor, key_counts: torch.Tensor,
                       H: int | None = None, W: int | None = None, pag: bool = False, cfg: bool = False, skip_first_layer: bool = False) -> torch.Tensor:
        """:meth:`forward` on a padded condition (cond [B, L, dim], key_counts int32 [B]): no host synchronisation, capturable."""
        return self._run(hidden_states, timestep, lambda b: b._cross_padded(cond, key_counts), H, W, pag, cfg, skip_first_layer)

    def _layer_pag(self, idx: int, pag: bool) -> bool:
        if not 0 <= idx < self.num_layers:
            raise IndexError(f"SanaModel: layer {idx} of {self.num_layers}")
        return bool(pag) and idx in self.pag_layers

    def forward_layer(self, idx: int, hidden_states, encoder_hidden_states, timestep, cu_seqlens_img, cu_seqlens_txt, H=None, W=None,
                      pag: bool = False, cfg: bool = False) -> torch.Tensor:
        """One block on its own (reference: ``QuantizedSanaModel::forward_layer``, nunchaku/csrc/sana.h): it computes its own modulation."""
        return self.transformer_blocks[idx](hidden_states, encoder_hidden_states, timestep, cu_seqlens_img, cu_seqlens_txt, H, W,
                                            self._layer_pag(idx, pag), cfg)

    def forward_layer_padded(self, idx: int, hidden_states, cond, timestep, key_counts, H=None, W=None, pag: bool = False, cfg: bool = False) -> torch.Tensor:
        return self.transformer_blocks[idx].forward_padded(hidden_states, cond, timestep, key_counts, H, W, self._layer_pag(idx, pag), cfg)


def convert_sana_state_dict(sd: dict) -> dict:
    """A whole checkpoint: the legacy-name mapping of :func:`convert_sana_attention_state_dict` under ``transformer_blocks.{i}.{attn,cross_attn,ff}.``;
    ``transformer_blocks.{i}.scale_shift_table`` and every key outside ``transformer_blocks.`` pass through.  The quantised part of the result loads
    into :class:`SanaModel` with ``strict=True``."""
    inside = {k: v for k, v in sd.items() if k.startswith("transformer_blocks.") and k.split(".")[2:3] in (["attn"], ["cross_attn"], ["ff"])}
    new = convert_sana_attention_state_dict(inside)
    new.update((k, v) for k, v in sd.items() if k not in inside)
    return new
