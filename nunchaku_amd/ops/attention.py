"""Attention over the packed QKV buffer (role of the reference's ``nunchaku-fp16`` attention processor:
nunchaku/models/attention_processors/flux.py:62-137 -> ops.attention_fp16, src/kernels/zgemm/attention.cu:11-94)."""

from __future__ import annotations

import math

import torch

from .._C import ops
from ..mode import alloc_lora_act, lora_act_words


def alloc_qkv(tokens: int, heads: int, dtype: torch.dtype, device, head_dim: int = 128):
    """Buffers one attention layer needs: ``qkv`` [tokens, 3*H*D] (the V third stays unused) and ``vt`` [H*D, tokens]."""
    qkv = torch.empty(tokens, 3 * heads * head_dim, dtype=dtype, device=device)
    vt = torch.empty(heads * head_dim, tokens, dtype=dtype, device=device)
    return qkv, vt


def q_prescale(head_dim: int = 128, scale: float | None = None) -> float:
    """The factor a QKV GEMM applies to Q (``fused_qkv_norm_rottary(..., q_scale=)``) so that the attention kernel needs no per-score
    scaling: ``scale * log2(e)``.  Pass ``q_prescaled=True`` to the attention call that reads that buffer."""
    return (1.0 / math.sqrt(head_dim) if scale is None else scale) * 1.4426950408889634


def kv_valid_ranges(t_first: int, t_second: int = 0, pad: int = 256):
    """Key ranges of a [first | second] token sequence whose streams are each padded to ``pad`` rows (what the grouped launches need: every
    stream starts on a 256-row boundary): ``None`` when nothing is padded, ``(n,)`` when only the tail is, ``(n0, start1, end1)`` when the
    padding of the first stream sits in the middle -- the forms ``ops.attention(kv_valid=...)`` takes."""
    p_first = (t_first + pad - 1) // pad * pad
    p_second = (t_second + pad - 1) // pad * pad
    if p_first == t_first and p_second == t_second:
        return None
    if t_second == 0:
        return (t_first,)
    if p_first == t_first:
        return (t_first + t_second,)
    return (t_first, p_first, p_first + t_second)


def attention_packed(qkv: torch.Tensor, vt: torch.Tensor, heads: int, out: torch.Tensor | None = None,
                     scale: float | None = None, zero_floats: int = 0, q_prescaled: bool = False, kv_valid=None):
    """``softmax(scale * Q K^T) V`` per head, reading Q and K in place from the fused QKV GEMM output
    ``qkv`` [L, 3*H*128] and V from its transposed side output ``vt`` [H*128, L]; returns ``[L, H*128]``
    token-major (the layout the output projection's quantiser reads).  No transposes, no copies.
    ``zero_floats`` > 0: also returns a ``ZeroPool`` of that many fp32 zeros cleared by the same launch (the low-rank
    accumulators of the output projections' quantisers): ``(out, pool)``.  ``kv_valid``: the real key rows of a padded buffer
    (:func:`kv_valid_ranges`); the other keys get probability 0."""
    L, three_hd = qkv.shape
    D = three_hd // (3 * heads)
    if three_hd != 3 * heads * D or tuple(vt.shape) != (heads * D, L):
        raise ValueError("attention_packed: expected qkv [L, 3*H*D] and vt [H*D, L]")
    if out is None:
        out = torch.empty(L, heads * D, dtype=qkv.dtype, device=qkv.device)
    q = qkv[:, : heads * D].unflatten(1, (heads, D))
    k = qkv[:, heads * D : 2 * heads * D].unflatten(1, (heads, D))
    zwords = zero_floats * lora_act_words()
    zero = torch.empty((zwords + 3) // 4 * 4, dtype=torch.float32, device=qkv.device) if zero_floats > 0 else None
    ops.attention(q, k, vt.unflatten(0, (heads, D)), out.unflatten(1, (heads, D)), 1.0 / math.sqrt(D) if scale is None else scale, zero,
                  q_prescaled=q_prescaled, kv_valid=kv_valid)
    if zero_floats > 0:
        from .elementwise import ZeroPool

        return out, ZeroPool(zero)
    return out


def attention_packed_quantized(qkv: torch.Tensor, vt: torch.Tensor, heads: int, lin, lin_first=None, split_rows: int = 0,
                               pool=None, scale: float | None = None, q_prescaled: bool = False, kv_valid=None):
    """Attention whose epilogue emits the quantised input of the output projection ``lin`` directly (codes, scales and
    low-rank down projection: what ``lin.quantize(attention_packed(...))`` would return, without the 16-bit round trip).
    Joint attention: rows ``< split_rows`` belong to ``lin_first`` (text), the rest to ``lin``.  ``pool``: a ZeroPool for
    the low-rank accumulator.  Returns ``(codes, scales, lora_act)`` or None when the shapes do not allow it."""
    L, three_hd = qkv.shape
    D = three_hd // (3 * heads)
    K, R = heads * D, lin.rank
    if D != 128 or L % 256 or K != lin.in_features or R > 256 or R % 16 or (lin_first is not None and (
            lin_first.rank != R or lin_first.in_features != K or split_rows % 256 or not 0 < split_rows < L)):
        return None
    lin._ensure_layout()
    dev = qkv.device
    act = torch.empty(L, K * 3 // 4, dtype=torch.uint8, device=dev)
    asc = torch.empty(K // 64, L, dtype=qkv.dtype, device=dev)
    lact, zeroed = alloc_lora_act(L, R, dev, pool)
    if not zeroed:
        lact.zero_()
    quant = dict(act=act, ascales=asc, lora_act=lact, R=R)
    if lin_first is not None:  # first parameter set = the rows that come first (text)
        lin_first._ensure_layout()
        quant.update(smooth=lin_first.smooth_factor, lora_down=lin_first.proj_down, smooth2=lin.smooth_factor,
                     lora_down2=lin.proj_down, split_rows=split_rows)
    else:
        quant.update(smooth=lin.smooth_factor, lora_down=lin.proj_down)
    q = qkv[:, : heads * D].unflatten(1, (heads, D))
    k = qkv[:, heads * D : 2 * heads * D].unflatten(1, (heads, D))
    ops.attention(q, k, vt.unflatten(0, (heads, D)), None, 1.0 / math.sqrt(D) if scale is None else scale, None, quant, q_prescaled=q_prescaled,
                  kv_valid=kv_valid)
    return act, asc, lact


def ip_attention(qkv_or_q: torch.Tensor, k_ip: torch.Tensor, v_ip: torch.Tensor, heads: int, out: torch.Tensor | None = None,
                 scale: float | None = None, out_scale: float = 1.0, q_prescaled: bool = False):
    """Image-prompt cross-attention of IP-Adapter: ``round16(out_scale * round16(softmax(scale * Q K_ip^T) V_ip))`` per head, one launch.
    ``qkv_or_q``: the packed ``[T, 3*H*128]`` output of a fused QKV GEMM (its Q third is read in place, no copy) or a ``[T, H*128]`` Q;
    ``k_ip`` / ``v_ip``: ``[N, H*128]`` as the adapter's ``nn.Linear`` projections wrote them, ``1 <= N <= 256``.  ``out_scale`` (the
    adapter's strength, a Python float) multiplies in fp32 as torch does for ``scale * tensor``.  Returns ``[T, H*128]`` token-major."""
    T, width = qkv_or_q.shape
    hd = k_ip.shape[-1]
    if hd % heads or width not in (hd, 3 * hd):
        raise ValueError("ip_attention: expected q [T, H*D] or qkv [T, 3*H*D] and k_ip / v_ip [N, H*D]")
    D = hd // heads
    if out is None:
        out = torch.empty(T, hd, dtype=qkv_or_q.dtype, device=qkv_or_q.device)
    ops.ip_attention(qkv_or_q[:, :hd].unflatten(1, (heads, D)), k_ip.reshape(-1, hd) if k_ip.dim() != 2 else k_ip,
                     v_ip.reshape(-1, hd) if v_ip.dim() != 2 else v_ip, out.unflatten(1, (heads, D)),
                     1.0 / math.sqrt(D) if scale is None else scale, out_scale=out_scale, q_prescaled=q_prescaled)
    return out


def pulid_ca(x: torch.Tensor, fold, out_scale: float = 1.0, stats: torch.Tensor | None = None, out: torch.Tensor | None = None,
             return_probs: bool = False, acc: torch.Tensor | None = None, o_acc: torch.Tensor | None = None):
    """PuLID's identity cross-attention with ``to_q`` and ``to_out`` folded into the keys and values (``svdq_pulid_ca``):
    ``round16(out_scale * round16(sum_h softmax(rstd (x . a_fold_h - mean colsum_h) + cbias_h) . b_fold_h))``.
    ``x``: ``[T, C]`` or ``[1, T, C]`` with any row stride -- the UN-normalised image stream; ``fold``: the record of
    ``models.pulid.PerceiverAttentionCA.fold`` (``a_fold``, ``b_fold`` ``[H * 32, C]``, ``colsum``, ``cbias`` ``[H * 32]`` float32, ``tokens``);
    ``stats``: float32 ``[T, 2]`` (mean, rstd) of the rows of ``x`` for eps = 1e-5 -- None: one stats-only ``residual_gate_stats`` launch
    computes them.  ``out_scale`` (``id_weight``, a Python float) multiplies in fp32.  Returns ``out`` in the shape of ``x``; with
    ``return_probs`` also the 16-bit probabilities ``[T, H * 32]`` (the call's workspace).  ``acc`` / ``o_acc``: float32 ``[T, H * 32]`` /
    ``[T, C]`` tensors that receive the two accumulators (tests)."""
    x2 = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])
    T, C = x2.shape
    if stats is None:
        from .elementwise import residual_gate_stats

        stats = residual_gate_stats(x2, eps=1e-5)[1]
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    probs = torch.empty(T, fold.a_fold.shape[0], dtype=x.dtype, device=x.device)
    ops.pulid_ca(x2, stats, fold.a_fold, fold.colsum, fold.cbias, fold.b_fold, probs, out if out.dim() == 2 else out.view(-1, C),
                 fold.tokens, out_scale=out_scale, acc=acc, o_acc=o_acc)
    return (out, probs) if return_probs else out


def linear_attention(qkv: torch.Tensor, heads: int, out: torch.Tensor | None = None, tokens: int | None = None, return_vk: bool = False,
                     eps: float = 1e-6):
    """SANA's ReLU linear attention over the packed output of the QKV projection, read in place (no copies): per batch element and head
    (head_dim 32), ``vk = [V | 1]^T relu(K)`` summed over the tokens in fp32 and ``out = relu(Q) vk[:32]^T / (relu(Q) . vk[32] + eps)``,
    rounded once.  ``qkv``: ``[B, T, 3*H*32]``, or ``[B*T, 3*H*32]`` with ``tokens=T`` (one batch element without it); the columns are the
    reference's: Q of head h at ``32 h``, then K and V of head h at ``H*32 + 64 h`` and ``H*32 + 64 h + 32``.  Any row and batch stride
    that keeps rows 16-byte aligned.  Returns ``out`` in the leading shape of ``qkv`` with ``H*32`` columns, token-major (what the output
    projection's quantiser reads); with ``return_vk`` also the float32 ``[B, H, 33, 32]`` sums.  No atomics: bit-equal from call to call."""
    if qkv.dim() == 3:
        B, T = qkv.shape[:2]
        packed = qkv
    elif qkv.dim() == 2:
        T = qkv.shape[0] if tokens is None else int(tokens)
        if T < 1 or qkv.shape[0] % T:
            raise ValueError("linear_attention: the rows of a [B*T, 3*H*D] qkv must be a multiple of tokens")
        B = qkv.shape[0] // T
        packed = qkv.unflatten(0, (B, T))
    else:
        raise ValueError("linear_attention: expected qkv [B, T, 3*H*D] or [B*T, 3*H*D]")
    hd = packed.shape[-1] // 3
    D = hd // heads
    if packed.shape[-1] != 3 * heads * D or (tokens is not None and qkv.dim() == 3 and int(tokens) != T):
        raise ValueError("linear_attention: expected qkv [B, T, 3*H*D] or [B*T, 3*H*D] (+ tokens)")
    if out is None:
        out = torch.empty(*qkv.shape[:-1], hd, dtype=qkv.dtype, device=qkv.device)
    if tuple(out.shape) not in ((B, T, hd), (B * T, hd)):
        raise ValueError("linear_attention: out must be [B, T, H*D] or [B*T, H*D]")
    out4 = (out if out.dim() == 3 else out.unflatten(0, (B, T))).unflatten(-1, (heads, D))
    vk = torch.empty(B, heads, D + 1, D, dtype=torch.float32, device=qkv.device) if return_vk else None
    ops.linear_attention(packed[..., :hd].unflatten(-1, (heads, D)), packed[..., hd:].unflatten(-1, (heads, 2 * D)), out4, vk, eps)
    return (out, vk) if return_vk else out


CROSS_ATTENTION_MAX_KEYS = 320  # keys per sample: K and V of one (sample, head) stay in LDS (csrc/cross_attention.hip, XA_MAX_KEYS)


def cross_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, head_dim: int, *, cu_seqlens: torch.Tensor | None = None,
                    key_offsets: torch.Tensor | None = None, key_counts: torch.Tensor | None = None, max_keys: int | None = None,
                    scale: float | None = None, out: torch.Tensor | None = None):
    """SANA's text cross-attention, one launch: per sample ``b`` and head, ``round16(softmax(scale * Q_b K_b^T) V_b)`` where ``K_b`` / ``V_b`` are
    the rows of ``k`` / ``v`` in sample ``b``'s key range.  ``head_dim`` 72, 112 or 128; ``scale`` defaults to ``head_dim ** -0.5``.

    ``q``: ``[B, T, >= H*D]`` (the output of ``q_linear``, whose rows may be wider than ``H*D``: the first ``H*D`` columns are read in place) or,
    with ``cu_seqlens``, ``[B*T, >= H*D]`` with ``B = len(cu_seqlens) - 1``.  ``k`` / ``v``: ``[Nrows, H*D]``; they may be the two column halves of
    one ``[Nrows, 2*H*D]`` tensor (what ``kv_linear`` wrote), no copy.  A ``[B, L, H*D]`` pair is taken as its ``[B*L, H*D]`` rows.

    The key ranges, exactly one of
      * ``cu_seqlens``: int32 ``[B + 1]``, flash-attention's packed layout: sample ``b`` owns rows ``cu[b] .. cu[b+1]``;
      * ``key_offsets`` and ``key_counts``: int32 ``[B]`` each; a padded ``[B, L, .]`` condition is ``offsets = b * L, counts = mask.sum(1)``.
    They live on q's device and are read by the kernel only: no host synchronisation, the call can be captured in a graph.  ``max_keys`` is
    the host's bound on any count (default ``k.shape[0]``), at most 320; the kernel clamps a count to ``[0, max_keys]`` and cuts a range at the
    last row of ``k``.  A sample without keys gets zero rows (a ``k`` without rows: all of them).

    Returns ``out`` in the leading shape of ``q`` with ``H*D`` columns, token-major; a given ``out`` may be a column slice of a wider buffer."""
    hd = heads * head_dim
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"cross_attention: {name} must be a tensor")
        if t.dtype not in (torch.bfloat16, torch.float16):
            raise TypeError(f"cross_attention: {name} must be bfloat16 or float16, got {t.dtype}")
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"cross_attention: k ({k.dtype}) and v ({v.dtype}) must have q's dtype {q.dtype}")
    if (cu_seqlens is None) == (key_offsets is None and key_counts is None):
        raise ValueError("cross_attention: pass either cu_seqlens or the key_offsets / key_counts pair (exactly one of the two forms)")
    if cu_seqlens is None and (key_offsets is None or key_counts is None):
        raise ValueError("cross_attention: key_offsets and key_counts go together")
    for name, t in (("cu_seqlens", cu_seqlens), ("key_offsets", key_offsets), ("key_counts", key_counts)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise TypeError(f"cross_attention: {name} must be an int32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if t.device != q.device:
            raise ValueError(f"cross_attention: {name} must live on q's device {q.device}, got {t.device}")
        if t.dim() != 1:
            raise ValueError(f"cross_attention: {name} must be one-dimensional, got {tuple(t.shape)}")
    if cu_seqlens is not None:
        B = cu_seqlens.shape[0] - 1
        if B < 1:
            raise ValueError("cross_attention: cu_seqlens must have B + 1 >= 2 entries")
        key_offsets, key_counts = cu_seqlens[:-1], cu_seqlens[1:] - cu_seqlens[:-1]
    else:
        B = key_offsets.shape[0]
        if B < 1 or key_counts.shape[0] != B:
            raise ValueError(f"cross_attention: key_offsets {tuple(key_offsets.shape)} and key_counts {tuple(key_counts.shape)} must both be [B]")
    if q.dim() == 2 and cu_seqlens is not None and q.shape[0] % B == 0 and q.shape[0] >= B:
        q3 = q.unflatten(0, (B, q.shape[0] // B))
    elif q.dim() == 3 and q.shape[0] == B:
        q3 = q
    else:
        raise ValueError(f"cross_attention: q must be [B, T, >= H*D] (or [B*T, >= H*D] with cu_seqlens) with B={B}, got {tuple(q.shape)}")
    T = q3.shape[1]
    if q3.shape[-1] < hd or T < 1:
        raise ValueError(f"cross_attention: q must have at least heads * head_dim = {hd} columns and one row, got {tuple(q.shape)}")
    if k.dim() == 3 and v.dim() == 3:
        k, v = k.flatten(0, 1), v.flatten(0, 1)
    if k.dim() != 2 or k.shape[-1] != hd or tuple(v.shape) != tuple(k.shape):
        raise ValueError(f"cross_attention: k and v must be [Nrows, heads * head_dim = {hd}] of one shape, got {tuple(k.shape)} and {tuple(v.shape)}")
    if max_keys is None:
        max_keys = k.shape[0]
    if out is None:
        out = torch.empty(*q.shape[:-1], hd, dtype=q.dtype, device=q.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != q.dtype or out.device != q.device or tuple(out.shape) != (*q.shape[:-1], hd):
        raise ValueError(f"cross_attention: out must be a {q.dtype} tensor of shape {(*q.shape[:-1], hd)} on {q.device}, got "
                         f"{getattr(out, 'dtype', None)} {tuple(getattr(out, 'shape', ()))}")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not t.is_cuda:
            raise ValueError(f"cross_attention: {name} must be a GPU tensor (there is no CPU path)")
    if k.shape[0] == 0:  # no key rows at all: every range is empty (an empty tensor has no address to hand to the library)
        return out.zero_()
    out3 = out if out.dim() == 3 else out.unflatten(0, (B, T))
    ops.cross_attention(q3[..., :hd].unflatten(-1, (heads, head_dim)), k, v, out3.unflatten(-1, (heads, head_dim)),
                        key_offsets.contiguous(), key_counts.contiguous(), int(max_keys), head_dim ** -0.5 if scale is None else scale)
    return out


def attention_d64(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float | None = None, out: torch.Tensor | None = None):
    """Stable Diffusion XL's attention, one launch: per sample and head, ``round16(softmax(scale * Q K^T) V)`` at head dimension 64, no mask.

    ``q``: ``[B, T, H*64]``, ``k`` / ``v``: ``[B, N, H*64]``, or all three 2-D (one sample).  Each may be a column slice of a wider buffer: the
    thirds of a packed ``[B, T, 3*H*64]`` QKV projection and the outputs of ``to_k`` / ``to_v`` are read in place, without a ``chunk``, a
    ``view`` / ``transpose`` copy or a transposed V.  ``scale`` defaults to ``64 ** -0.5``.  Other head sizes raise ``NotImplementedError``;
    what the library rejects (strides, alignment, an ``out`` that overlaps an input) raises ``ValueError``.

    Returns ``out`` in the leading shape of ``q`` with ``H*64`` columns, token-major (what ``to_out[0]``'s quantiser reads); a given ``out``
    may be a column slice of a wider buffer.  No synchronisation and no allocation beyond ``out``."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"attention_d64: {name} must be a tensor")
        if t.dtype not in (torch.bfloat16, torch.float16):
            raise TypeError(f"attention_d64: {name} must be bfloat16 or float16, got {t.dtype}")
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"attention_d64: k ({k.dtype}) and v ({v.dtype}) must have q's dtype {q.dtype}")
    if q.dim() not in (2, 3) or k.dim() != q.dim() or v.dim() != q.dim():
        raise ValueError(f"attention_d64: q, k and v must all be [B, rows, H*64] or all [rows, H*64], got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    hd = q.shape[-1]
    if heads < 1 or hd % heads:
        raise ValueError(f"attention_d64: {hd} columns are not a multiple of heads={heads}")
    head_dim = hd // heads
    if head_dim != 64:
        raise NotImplementedError(f"attention_d64: head_dim={head_dim}: 64 is implemented ({hd} columns, {heads} heads)")
    if k.shape[-1] != hd or tuple(v.shape) != tuple(k.shape) or k.shape[:-2] != q.shape[:-2] or q.shape[-2] < 1 or k.shape[-2] < 1:
        raise ValueError(f"attention_d64: expected q [B, T, {hd}] and k / v [B, N, {hd}] of one batch size with T, N >= 1, got {tuple(q.shape)}, "
                         f"{tuple(k.shape)}, {tuple(v.shape)}")
    if out is None:
        out = torch.empty(*q.shape[:-1], hd, dtype=q.dtype, device=q.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != q.dtype or out.device != q.device or tuple(out.shape) != tuple(q.shape):
        raise ValueError(f"attention_d64: out must be a {q.dtype} tensor of shape {tuple(q.shape)} on {q.device}, got "
                         f"{getattr(out, 'dtype', None)} {tuple(getattr(out, 'shape', ()))}")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not t.is_cuda:
            raise ValueError(f"attention_d64: {name} must be a GPU tensor (there is no CPU path)")
    q4, k4, v4, o4 = ((t if t.dim() == 3 else t.unsqueeze(0)).unflatten(-1, (heads, 64)) for t in (q, k, v, out))
    ops.attention_d64(q4, k4, v4, o4, 64 ** -0.5 if scale is None else scale)
    return out


def qk_norm_rope(qkv: torch.Tensor, heads: int, tokens: int | None = None, *, norm_q: torch.Tensor | None = None, norm_k: torch.Tensor | None = None,
                 freqs_cis: torch.Tensor | None = None, vt: torch.Tensor | None = None, eps: float = 1e-5, want_rstd: bool = False):
    """Z-Image's step between the QKV projection and the attention, for ONE sample, in one launch (``svdq_qk_norm_rope``): per token and head
    the RMSNorm of Q and of K over the 128 values of the head (``norm_q`` / ``norm_k``: the ``[128]`` weights, None for no normalisation), then
    the rotation of the pairs ``(2i, 2i + 1)`` by ``freqs_cis[t, i]`` (None: no rotation), one 16-bit rounding per torch operation of the
    reference processor.  ``qkv``: ``[L, 3 * H * 128]`` with any row stride, whose first ``tokens`` rows (default: all) are real; its Q and K
    thirds are rewritten IN PLACE.  ``freqs_cis``: complex64 ``[tokens, 64]`` as the pipeline makes it, or its float32 ``[tokens, 64, 2]``
    ``torch.view_as_real``.  ``vt``: a ``[H * 128, >= L]`` buffer that gets V transposed in columns ``[0, tokens)`` and zeros in
    ``[tokens, L)`` (``L`` a multiple of 128: what ``attention_packed(qkv, vt[:, :L], heads, kv_valid=(tokens,))`` then reads), None for none.
    Returns ``qkv``, or ``(qkv, rstd)`` with ``want_rstd``: the float32 ``[tokens, 2 * H]`` reciprocal RMS values (Q heads, then K heads)."""
    op = "qk_norm_rope"
    if not isinstance(qkv, torch.Tensor) or qkv.dim() != 2:
        raise ValueError(f"{op}: qkv must be one sample's [L, 3 * H * 128] tensor")
    if qkv.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"{op}: qkv must be bfloat16 or float16, got {qkv.dtype}")
    L, width = qkv.shape
    if heads < 1 or width != 3 * heads * 128:
        raise NotImplementedError(f"{op}: head_dim 128 is implemented: {width} columns are not 3 * heads={heads} * 128")
    T = L if tokens is None else int(tokens)
    if not 1 <= T <= L:
        raise ValueError(f"{op}: tokens={T} must be within the {L} rows of qkv")
    for name, t in (("norm_q", norm_q), ("norm_k", norm_k)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != qkv.dtype or tuple(t.shape) != (128,)):
            raise ValueError(f"{op}: {name} must be a {qkv.dtype} [128] tensor")
    freqs = None
    if freqs_cis is not None:
        if not isinstance(freqs_cis, torch.Tensor):
            raise TypeError(f"{op}: freqs_cis must be a tensor")
        freqs = torch.view_as_real(freqs_cis) if freqs_cis.is_complex() else freqs_cis
        if freqs.dtype != torch.float32 or tuple(freqs.shape) != (T, 64, 2):
            raise ValueError(f"{op}: freqs_cis must be complex64 [{T}, 64] or float32 [{T}, 64, 2], got {freqs_cis.dtype} {tuple(freqs_cis.shape)}")
        freqs = freqs.contiguous()
    if vt is not None:
        if not isinstance(vt, torch.Tensor) or vt.dtype != qkv.dtype or vt.dim() != 2 or vt.shape[0] != heads * 128 or vt.shape[1] < L:
            raise ValueError(f"{op}: vt must be a {qkv.dtype} [{heads * 128}, >= {L}] tensor")
        if L % 128:
            raise ValueError(f"{op}: with vt the rows of qkv are the padded length of the attention: {L} is not a multiple of 128")
    for name, t in (("qkv", qkv), ("norm_q", norm_q), ("norm_k", norm_k), ("freqs_cis", freqs), ("vt", vt)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"{op}: {name} must be a GPU tensor (there is no CPU path)")
    rstd = torch.empty(T, 2 * heads, dtype=torch.float32, device=qkv.device) if want_rstd else None
    ops.qk_norm_rope(qkv, None if norm_q is None else norm_q.contiguous(), None if norm_k is None else norm_k.contiguous(), freqs, vt, rstd,
                     T, L, heads, eps=eps)
    return (qkv, rstd) if want_rstd else qkv
