"""W4A4 GEMM wrapper (reference: nunchaku/ops/gemm.py:12-160).  Keyword names and order are the reference's;
everything after ``attn_tokens`` is an extension of this library."""

from __future__ import annotations

import math

import torch

from .._C import ops

T = torch.Tensor


def svdq_gemm_w4a4_cuda(
    act: T, wgt: T, out: T | None = None, qout: T | None = None,            # operand images, 16-bit / requantised output
    ascales: T | None = None, wscales: T | None = None, oscales: T | None = None, poolout: T | None = None,
    lora_act_in: T | None = None, lora_up: T | None = None,                 # low-rank branch of THIS layer
    lora_down: T | None = None, lora_act_out: T | None = None,              # ... of the NEXT layer (GELU_QUANT epilogue)
    norm_q: T | None = None, norm_k: T | None = None, rotary_emb: T | None = None,   # RMSNorm + RoPE epilogue
    bias: T | None = None, smooth_factor: T | None = None,
    out_vk: T | None = None, out_linearattn: T | None = None,               # SANA LiteLA: fp32 [B, H, 33, 32] sums / relu(Q) [B, T_pad, N/3]
    act_unsigned: bool = False, lora_scales: list[float] | None = None, fuse_silu: bool = False,
    fp4: bool = False, alpha: float | None = 1.0, wcscales: T | None = None,          # NVFP4 only
    out_q: T | None = None, out_k: T | None = None, out_v: T | None = None, attn_tokens: int = 0,
    out_vt: T | None = None, lora_act_zeroed: bool = False, second: dict | None = None, split_rows: int = 0,
    q_scale: float = 0.0,
) -> None:
    """Fused W4A4 GEMM + low-rank correction; results are written in place into ``out`` or, for the
    GELU+requantise fusion, into ``qout`` / ``oscales`` / ``lora_act_out``.  Extensions: ``out_vt`` (transposed V side
    output of the RoPE epilogue), ``lora_act_zeroed`` (skip the clear of ``lora_act_out``), ``second`` / ``split_rows``
    (a second weight set for the rows from ``split_rows`` on: two streams in one launch), ``q_scale`` (RoPE epilogue: the Q third
    times this factor before its rounding to 16-bit -- for ``ops.attention(q_prescaled=True)``)."""
    if lora_scales is None:  # one scale per 16 ranks, all ones (reference :125-127)
        lora_scales = [1.0] * math.ceil((0 if lora_up is None else lora_up.shape[1]) / 16)
    ops.gemm_w4a4(
        act, wgt, out, qout, ascales, wscales, oscales, poolout, lora_act_in, lora_up, lora_down, lora_act_out,
        norm_q, norm_k, rotary_emb, bias, smooth_factor, out_vk, out_linearattn, act_unsigned, lora_scales,
        fuse_silu, fp4, 1.0 if alpha is None else alpha, wcscales, out_q, out_k, out_v, attn_tokens,
        out_vt, lora_act_zeroed, second, split_rows, q_scale,
    )


AWQ_MULTI_MODES = {"concat": False, "gated_gelu_new": True}


def gemm_awq_multi(x: T, weights, mode: str = "concat", out: T | None = None) -> T:
    """One 16-bit ``x [..., K]`` against 1 to 3 AWQ W4A16 weight sets (group 128) in ONE launch (``svdq_gemm_awq_multi``).  ``weights``: a
    sequence of ``W4Linear`` modules or ``(qweight, scales, scaled_zeros, bias or None)`` tuples.

    * ``mode="concat"``: ``[..., sum N_i]``, set i in columns ``[sum_{j<i} N_j, ...)``, every element what ``ops.gemm_awq`` writes for its
      set (bit for bit where neither launch splits K) -- the T5 encoder's q / k / v as one buffer whose column thirds the attention reads.
    * ``mode="gated_gelu_new"`` (two sets of equal N): ``[..., N] = round16(round16(gelu_new(y_0)) * y_1)`` with ``y_i`` the two 16-bit GEMM
      results -- T5's gated-GELU feed-forward; the ``[..., 2N]`` intermediate is never written.

    ``out``: None, or a tensor of the result's shape to write into (unit column stride, uniformly strided rows: a column slice will do)."""
    if mode not in AWQ_MULTI_MODES:
        raise ValueError(f"gemm_awq_multi: mode={mode!r} (one of {sorted(AWQ_MULTI_MODES)})")
    sets = []
    for w in weights:
        if isinstance(w, (tuple, list)):
            if len(w) != 4:
                raise ValueError("gemm_awq_multi: a weight set is (qweight, scales, scaled_zeros, bias or None)")
            sets.append(tuple(w))
        else:
            if getattr(w, "group_size", None) != 128:
                raise NotImplementedError(f"gemm_awq_multi: group_size={getattr(w, 'group_size', None)} (the AWQ GEMM kernels implement 128)")
            sets.append((w.qweight, w.scales, w.scaled_zeros, w.bias))
    return ops.gemm_awq_multi(x, sets, AWQ_MULTI_MODES[mode], out)


def svdq_gemm_mxfp4(act: T, wgt: T, ascales: T, wscales: T, out: T | None = None, lora_act_in: T | None = None, lora_up: T | None = None,
                    bias: T | None = None, lora_scales: list[float] | None = None, rows: int | None = None,
                    qout: T | None = None, oscales: T | None = None, lora_down: T | None = None, lora_act_out: T | None = None,
                    smooth_factor: T | None = None, lora_act_zeroed: bool = False,
                    norm_q: T | None = None, norm_k: T | None = None, rotary_emb: T | None = None, out_vt: T | None = None,
                    q_scale: float = 0.0, glu: str | None = None) -> T | None:
    """MXFP4 W4A4 GEMM, plain epilogue: ``out[:rows] = A4 W4^T`` with both E8M0 block scales ``+ round16(lora_act_in * lora_scales) lora_up^T + bias``,
    one rounding to the 16-bit dtype of ``lora_up`` / ``bias`` / ``out`` (bfloat16 when none is given).  ``act`` / ``ascales`` as
    :func:`ops.quantize.svdq_quantize_mxfp4` returns them, ``wgt`` ``[N, K/2]``, ``wscales`` uint8 ``[K/32, N]``; ``rows``: the valid rows M
    (default: all of ``act``'s).  Deterministic: two calls are bit-equal.

    With ``qout`` (uint8 ``[M_pad, N/2]``) the GELU_QUANT epilogue runs, keywords as in :func:`svdq_gemm_w4a4_cuda`: ``g = round16(gelu_tanh(
    that fp32 sum))``, and ``qout`` / ``oscales`` (uint8 ``[N/128, M_pad, 4]``) / ``lora_act_out`` (fp32 ``[M_pad, R_next]``) receive what
    ``svdq_quantize_mxfp4(g, lora_down=lora_down, smooth=smooth_factor)`` returns -- codes and scales bit for bit, the operands of the next
    ``svdq_gemm_mxfp4`` as they are.  ``lora_act_out`` is summed over the N/128 column tiles with fp32 atomics: for N > 128 it (and the next GEMM's
    output through it) depends on the order of the adds; it is cleared first unless ``lora_act_zeroed``.  ``out``, if given, receives ``g``
    (no ``out`` is allocated in this mode); returns ``out``.

    With ``rotary_emb`` (float32 ``[M_pad, 128]`` in ``pack_rotemb`` order) and ``norm_q`` / ``norm_k`` (``[128]``) the RMSNorm + RoPE epilogue of
    a QKV projection runs, ``N = 3 * heads * 128``, keywords as in :func:`svdq_gemm_w4a4_cuda`: per head, the Q and K thirds are
    ``rope(h * rsqrt(mean(h^2) + 1e-6) * norm)`` of that fp32 sum ``h`` with one rounding, Q times ``q_scale`` before it (0 = off); the V third
    is the plain output, and with ``out_vt`` (``[N/3, tokens]``, rows on 16 bytes) it is written transposed there instead of into ``out``.
    These keywords together with ``qout`` raise ``ValueError``.

    With ``glu`` (``"silu"`` for SwiGLU, ``"gelu"`` for the erf GEGLU) and ``qout`` the GLU_QUANT epilogue of a gated projection runs: ``wgt`` is
    ``[2 * Hd, K/2]`` with the value rows first (diffusers' ``chunk(2, -1)``), and with ``v``, ``g`` the two 16-bit column halves the plain launch
    would write, ``x = round16(v * round16(act(g)))`` -- the rounding points of :func:`ops.quantize.svdq_quantize_glu_halves`; ``qout``
    (``[M_pad, Hd/2]``) / ``oscales`` (``[Hd/128, M_pad, 4]``) / ``lora_act_out`` receive what ``svdq_quantize_mxfp4(x, lora_down=lora_down,
    smooth=smooth_factor)`` returns (``smooth_factor`` ``[Hd]``, ``lora_down`` ``[Hd, R_next]``), codes and scales bit for bit; ``out``, if given,
    receives ``x`` ``[M, Hd]``.  The ``[M, 2 * Hd]`` projection output is never written.  ``glu`` without ``qout``, or together with ``norm_q`` /
    ``norm_k`` / ``rotary_emb`` / ``out_vt``, raises ``ValueError``."""
    if glu is not None and (qout is None or any(t is not None for t in (norm_q, norm_k, rotary_emb, out_vt))):
        raise ValueError("svdq_gemm_mxfp4: glu= (the GLU_QUANT epilogue) needs qout and does not combine with norm_q, norm_k, rotary_emb or out_vt")
    if qout is not None and any(t is not None for t in (norm_q, norm_k, rotary_emb, out_vt)):
        raise ValueError("svdq_gemm_mxfp4: norm_q, norm_k, rotary_emb and out_vt (the RMSNorm+RoPE epilogue) do not combine with qout (GELU_QUANT)")
    M = act.shape[0] if rows is None else int(rows)
    if out is None and qout is None:
        ref = lora_up if lora_up is not None else bias
        out = torch.empty(M, wgt.shape[0], dtype=torch.bfloat16 if ref is None else ref.dtype, device=act.device)
    ops.gemm_mxfp4(act, wgt, out, ascales, wscales, lora_act_in, lora_up, bias, lora_scales, M,
                   qout=qout, oscales=oscales, lora_down=lora_down, lora_act_out=lora_act_out, smooth_factor=smooth_factor, lora_act_zeroed=lora_act_zeroed,
                   norm_q=norm_q, norm_k=norm_k, rotary_emb=rotary_emb, out_vt=out_vt, q_scale=q_scale, glu=glu)
    return out
