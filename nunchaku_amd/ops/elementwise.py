"""Element-wise glue of a transformer block with the next LayerNorm's statistics fused in (extension of the
reference surface; the reference's V2 blocks use torch ops here: transformer_flux_v2.py:118-342)."""

from __future__ import annotations

import torch

from .._C import ops
from ..mode import lora_act_words


class ZeroPool:
    """Scratch words (fp32-sized) cleared by a :func:`residual_gate_stats` pass, handed out in pieces to the quantiser /
    GELU_QUANT calls that follow it on the same stream (their low-rank accumulators need a zeroed buffer: this saves
    one memset launch each).  ``take`` returns None when the pool is exhausted -- the caller then clears its own."""

    def __init__(self, buf: torch.Tensor):
        self.buf, self.used = buf, 0

    def take(self, numel: int):
        n = (numel + 3) // 4 * 4  # keep every piece 16-byte aligned
        if self.used + n > self.buf.numel():
            return None
        piece = self.buf[self.used:self.used + numel]
        self.used += n
        return piece


def ln_pool(ln):
    """The :class:`ZeroPool` an ``ln`` tuple carries -- ``(stats, scale, shift[, pool])`` -- or None (no tuple, no 4th element)."""
    return ln[3] if ln is not None and len(ln) > 3 else None


def residual_gate_stats(res: torch.Tensor, a: torch.Tensor | None = None, gate: torch.Tensor | None = None,
                        b: torch.Tensor | None = None, inplace: bool = True, want_stats: bool = True, eps: float = 1e-6,
                        zero_floats: int = 0, clamp_fp16: bool = False):
    """``y = res + gate * (a [+ b])`` (one 16-bit rounding per torch op, as the reference's blocks; ``a`` None: ``y = res``) and the row
    statistics ``[rows, 2]`` float32 (mean, rstd) of ``y`` for a following ``quantize(..., ln=...)``.  ``clamp_fp16``: clip
    ``y`` to +-65504 when the dtype is fp16 (the reference's fp16 blocks do, transformer_flux_v2.py:254-255, 339-340).
    Tensors are ``[..., C]`` contiguous; returns ``(y, stats)`` or, with ``zero_floats`` > 0, ``(y, stats, ZeroPool)``
    where the pool holds that many fp32 zeros cleared in the same pass."""
    C = res.shape[-1]
    r2 = res.reshape(-1, C)
    out = None
    if a is not None:
        out = r2 if inplace else torch.empty_like(r2)
    stats = torch.empty(r2.shape[0], 2, dtype=torch.float32, device=res.device) if want_stats else None
    want_pool = zero_floats > 0
    zero_floats *= lora_act_words()  # the count is in lora_act elements: two words each in deterministic mode
    zero = torch.empty((zero_floats + 3) // 4 * 4, dtype=torch.float32, device=res.device) if zero_floats > 0 else None
    ops.residual_gate_stats(r2, None if a is None else a.reshape(-1, C), None if b is None else b.reshape(-1, C),
                            None if gate is None else gate.reshape(-1), out, stats, eps, zero, clamp_fp16=int(bool(clamp_fp16)))
    y = res if out is None else out.view(res.shape)
    if want_pool:
        return y, stats, ZeroPool(zero if zero is not None else torch.empty(0, dtype=torch.float32, device=res.device))
    return y, stats


def residual_gate_stats_pair(res_a, a_a, gate_a, res_b, a_b, gate_b, zero_floats: int = 0, eps: float = 1e-6, clamp_fp16_a: bool = False,
                             clamp_fp16_b: bool = False, inplace: bool = True):
    """Two independent gated residuals (the two streams of a joint block: same width, different row counts) and their
    statistics in ONE launch, both in place (``inplace`` False: into new tensors).  Returns ``(y_a, stats_a, y_b, stats_b[, ZeroPool])``."""
    C = res_a.shape[-1]
    ra, rb = res_a.reshape(-1, C), res_b.reshape(-1, C)
    oa, ob = (ra, rb) if inplace else (torch.empty_like(ra), torch.empty_like(rb))
    sa = torch.empty(ra.shape[0], 2, dtype=torch.float32, device=res_a.device)
    sb = torch.empty(rb.shape[0], 2, dtype=torch.float32, device=res_a.device)
    zf = zero_floats * lora_act_words()
    zero = torch.empty((zf + 3) // 4 * 4, dtype=torch.float32, device=res_a.device) if zf > 0 else None
    ops.residual_gate_stats(ra, a_a.reshape(-1, C), None, gate_a.reshape(-1), oa, sa, eps, zero,
                            second=(rb, a_b.reshape(-1, C), None, gate_b.reshape(-1), ob, sb),
                            clamp_fp16=int(bool(clamp_fp16_a)) | (2 if clamp_fp16_b else 0))
    if not inplace:
        res_a, res_b = oa.view(res_a.shape), ob.view(res_b.shape)
    if zero_floats > 0:
        return res_a, sa, res_b, sb, ZeroPool(zero if zero is not None else torch.empty(0, dtype=torch.float32, device=res_a.device))
    return res_a, sa, res_b, sb


def residual_add_pair(res_a, a_a, res_b, a_b, want_stats: bool = False, eps: float = 1e-6):
    """``res_a += a_a`` and ``res_b += a_b`` (one 16-bit add each, in place) in ONE launch, with the row statistics of both sums when
    ``want_stats``: a First-Block-Cache hit adds the stored residuals of the two streams this way.  Returns ``(stats_a, stats_b)``."""
    C = res_a.shape[-1]
    ra, rb = res_a.reshape(-1, C), res_b.reshape(-1, C)
    sa = torch.empty(ra.shape[0], 2, dtype=torch.float32, device=res_a.device) if want_stats else None
    sb = torch.empty(rb.shape[0], 2, dtype=torch.float32, device=res_a.device) if want_stats else None
    ops.residual_gate_stats(ra, a_a.reshape(-1, C), None, None, ra, sa, eps, None, second=(rb, a_b.reshape(-1, C), None, None, rb, sb))
    return sa, sb


class ResidualDiff:
    """The device record of a :func:`residual_diff` launch (``svdq_residual_diff_result``).  ``read()`` copies it to the host --
    that synchronises the stream, so it raises while the stream is being captured -- and keeps the values."""

    FIELDS = ("sum_diff", "sum_prev", "mean_diff", "mean_prev", "ratio")

    def __init__(self, record: torch.Tensor, dtype: torch.dtype):
        self.record, self.dtype, self._host = record, dtype, None

    def read(self) -> dict:
        if self._host is None:
            if self.record.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("residual_diff: the result record is read on the host, which synchronises the stream: "
                                   "not possible while the stream is being captured into a graph")
            self._host = dict(zip(self.FIELDS, self.record[:5].tolist()))
        return self._host

    @property
    def ratio(self) -> torch.Tensor:
        """the 16-bit quotient of the two 16-bit means, a 0-dim CPU tensor in the dtype of the compared tensors"""
        return torch.tensor(self.read()["ratio"], dtype=self.dtype)

    def is_similar(self, threshold: float) -> torch.Tensor:
        return self.ratio < threshold  # torch's comparison of a 16-bit tensor with a Python number


def _row_views(op: str, ref: torch.Tensor, **tensors) -> list:
    """The ``[rows, C]`` views of contiguous ``[..., C]`` tensors that hold what ``ref`` holds (None stays None)"""
    C, views = ref.shape[-1], []
    for name, t in tensors.items():
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{op}: {name} must be contiguous (row slices of a contiguous tensor are)")
        if t is not None and (t.shape[-1] != C or t.numel() != ref.numel()):
            raise ValueError(f"{op}: shapes differ: {name} {tuple(t.shape)} vs {tuple(ref.shape)}")
        views.append(None if t is None else t.view(-1, C))
    return views


def residual_diff(cur, base=None, prev=None, out=None, want_res: bool | None = None):
    """``r = cur - base`` (``base`` None: ``r = cur``) and, with ``prev``, the relative L1 distance ``mean|prev - r| / mean|prev|`` with
    the rounding points of the reference's 16-bit torch ops (caching/fbcache.py:275-277), in one pass over the tensors.
    Every argument is a ``[..., C]`` tensor or a sequence of up to two of them: two problems (the real text and image rows of a padded
    joint sequence) feed the same two sums.  Returns ``(r or None, ResidualDiff or None)``; ``r`` is ``out`` when given, else new
    (a list for two problems); ``want_res`` defaults to "when there is a base"."""
    def seq(x):
        return list(x) if isinstance(x, (list, tuple)) else [x]

    curs = seq(cur)
    n = len(curs)
    if not 1 <= n <= 2:
        raise ValueError("residual_diff: one or two problems")
    bases, prevs, outs = (seq(x) if x is not None else [None] * n for x in (base, prev, out))
    if not (len(bases) == len(prevs) == len(outs) == n):
        raise ValueError("residual_diff: base / prev / out must have as many entries as cur")
    if want_res is None:
        want_res = base is not None
    if want_res and base is None:
        raise ValueError("residual_diff: without a base the residual is cur itself")
    if want_res and out is None:
        outs = [torch.empty(c.shape, dtype=c.dtype, device=c.device) for c in curs]
    probs = [_row_views("residual_diff", c, cur=c, base=b, prev=p, out=o if want_res else None) for c, b, p, o in zip(curs, bases, prevs, outs)]
    rows = sum(p[0].shape[0] for p in probs)
    rec = None
    partials = result = None
    if prev is not None:
        partials = torch.empty(rows, 2, dtype=torch.float32, device=curs[0].device)
        result = torch.empty(8, dtype=torch.float32, device=curs[0].device)
        rec = ResidualDiff(result, curs[0].dtype)
    ops.residual_diff(*probs[0], partials=partials, result=result, second=probs[1] if n == 2 else None)
    res = None
    if want_res:
        res = outs if isinstance(cur, (list, tuple)) else outs[0]
    return res, rec


def modulated_diff(x, stats, scale, shift, prev=None, out=None, scratch=None):
    """``m = LayerNorm(x) * scale + shift`` with the rounding points of the quantiser's fused AdaLayerNormZero front end (``stats``: the
    ``[rows, 2]`` float32 (mean, rstd) of :func:`residual_gate_stats`; ``scale`` / ``shift``: ``[C]``, the scale with its +1) and, with
    ``prev``, the relative L1 distance ``mean|prev - m| / mean|prev|`` of TeaCache's decision (reference: caching/teacache.py:199-200) in
    the same pass.  ``x`` / ``prev`` / ``out`` are ``[..., C]`` contiguous tensors of one shape; ``out`` may be ``prev`` (one buffer kept
    across steps).  ``scratch``: ``(partials, record)`` of an earlier :func:`modulated_diff_scratch` call to reuse instead of allocating (the
    record of the earlier launch must have been read, or be of no interest, by then).  Returns ``(m, ResidualDiff or None)``; ``m`` is ``out``
    when given, else new."""
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    x2, prev2, out2 = _row_views("modulated_diff", x, x=x, prev=prev, out=out)
    rec = partials = result = None
    if prev is not None:
        partials, result = scratch if scratch is not None else modulated_diff_scratch(x2.shape[0], x.device)
        rec = ResidualDiff(result, x.dtype)
    ops.modulated_diff(x2, stats, scale.reshape(-1), shift.reshape(-1), prev2, out2, partials=partials, result=result)
    return out, rec


def modulated_diff_scratch(rows: int, device):
    """``(partials [rows, 2], record [8])`` float32: what a :func:`modulated_diff` launch with ``prev`` writes besides ``out``"""
    return torch.empty(rows, 2, dtype=torch.float32, device=device), torch.empty(8, dtype=torch.float32, device=device)


SANA_MSA = (0, 1, 2)  # rows (shift, scale, gate) of a SANA block's ``timestep + scale_shift_table`` for the linear attention
SANA_MLP = (3, 4, 5)  # ... and for the feed-forward (src/SanaModel.cpp:262)


def sana_glue(res: torch.Tensor, a: torch.Tensor | None = None, *, timestep: torch.Tensor | None = None, gate_table: torch.Tensor | None = None,
              gate_row: int | None = None, mod_table: torch.Tensor | None = None, scale_row: int | None = None, shift_row: int | None = None,
              channels: int | None = None, pad_to: int | None = None, out: torch.Tensor | bool | None = None,
              out_mod: torch.Tensor | bool | None = None, want_stats: bool = False, eps: float = 1e-6):
    """The glue pass of a SANA block in one launch (``svdq_sana_glue``; reference: src/SanaModel.cpp:234-322, nine launches per block there).

    ``res`` / ``a``: ``[B, T, >= channels]`` with unit stride on the last axis (a column slice of a wider buffer will do); ``timestep``: ``[B, 6, channels]``
    or ``[B, 6 * channels]``; the tables: ``[6, channels]``.  With ``mod(tab, i)[b] = clip(timestep[b, i] + tab[i])`` (one 16-bit rounding per
    operation throughout, ``clip`` to +-65504 for fp16 only)::

        t = res  |  clip(a + res)  |  clip(a * mod(gate_table, gate_row)[b] + res)          (no a | gate_row None | gate_row 0..5)
        out = t;   out_mod = clip(layer_norm(t) * (mod(mod_table, scale_row)[b] + 1) + mod(mod_table, shift_row)[b])

    ``channels`` defaults to ``res.shape[-1]``, ``pad_to`` to ``ceil(channels / 128) * 128``: both outputs are ``[B, T, pad_to]`` with zeros behind
    column ``channels``.  ``out`` / ``out_mod``: a tensor to write into (``out`` may be ``res``), True to allocate one, None / False for none;
    ``out_mod`` defaults to "when ``mod_table`` is given", ``out`` to "when ``a`` is given".  Returns ``(out, out_mod, stats)`` with None for what
    was not asked for; ``stats`` is the float32 ``[B * T, 2]`` (mean, rstd) of ``t``."""
    op = "sana_glue"
    if not isinstance(res, torch.Tensor) or res.dim() != 3:
        raise ValueError(f"{op}: res must be a [B, T, C] tensor")
    if res.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"{op}: res must be bfloat16 or float16, got {res.dtype}")
    B, T = res.shape[:2]
    C = res.shape[-1] if channels is None else int(channels)
    C_pad = (C + 127) // 128 * 128 if pad_to is None else int(pad_to)
    if C < 8 or C % 8 or C_pad % 8 or C_pad < C or res.shape[-1] < C or B < 1 or T < 1:
        raise ValueError(f"{op}: need channels={C} a multiple of 8 within res {tuple(res.shape)} and pad_to={C_pad} >= channels, a multiple of 8")
    if out is None:
        out = a is not None
    if out_mod is None:
        out_mod = mod_table is not None
    out = torch.empty(B, T, C_pad, dtype=res.dtype, device=res.device) if out is True else None if out is False else out
    out_mod = torch.empty(B, T, C_pad, dtype=res.dtype, device=res.device) if out_mod is True else None if out_mod is False else out_mod
    if out is None and out_mod is None and not want_stats:
        raise ValueError(f"{op}: nothing to do: none of out, out_mod and stats is asked for")
    if gate_row is not None and (a is None or gate_table is None or timestep is None):
        raise ValueError(f"{op}: a gate needs a, gate_table and timestep")
    if out_mod is not None and (mod_table is None or timestep is None or scale_row is None or shift_row is None):
        raise ValueError(f"{op}: out_mod needs timestep, mod_table, scale_row and shift_row")
    for name, row in (("gate_row", gate_row), ("scale_row", scale_row), ("shift_row", shift_row)):
        if row is not None and not 0 <= int(row) <= 5:
            raise ValueError(f"{op}: {name}={row}: the tables have rows 0..5")
    if not (eps >= 0.0) or eps == float("inf"):
        raise ValueError(f"{op}: eps={eps} must be finite and not negative")

    def row_stride(name, t, width):
        """the row stride of a [B, T, >= width] view whose samples lie T rows apart (0 for None)"""
        if t is None:
            return 0
        if not isinstance(t, torch.Tensor) or t.dtype != res.dtype:
            raise TypeError(f"{op}: {name} must be a {res.dtype} tensor like res")
        if t.device != res.device:
            raise ValueError(f"{op}: {name} must live on res's device {res.device}, got {t.device}")
        if t.dim() != 3 or t.shape[0] != B or t.shape[1] != T or t.shape[2] < width:
            raise ValueError(f"{op}: {name} must be [{B}, {T}, >= {width}], got {tuple(t.shape)}")
        s0, s1, s2 = t.stride()
        if s2 != 1 or (B > 1 and T > 1 and s0 != T * s1):
            raise ValueError(f"{op}: {name} must have unit stride on its last axis and hold its samples T rows apart")
        # (the strides of dimensions of size 1 are arbitrary in torch: the library gets the natural ones)
        return s1 if T > 1 else s0 if B > 1 else max(t.shape[2], width)

    if out is not None and out.shape[-1] != C_pad:
        raise ValueError(f"{op}: out must be [{B}, {T}, {C_pad}], got {tuple(out.shape)}")
    if out_mod is not None and (not isinstance(out_mod, torch.Tensor) or out_mod.shape[-1] != C_pad):
        raise ValueError(f"{op}: out_mod must be [{B}, {T}, {C_pad}], got {tuple(getattr(out_mod, 'shape', ()))}")
    lds = (row_stride("res", res, C), row_stride("a", a, C), row_stride("out", out, C_pad), row_stride("out_mod", out_mod, C_pad))
    if timestep is not None:
        if not isinstance(timestep, torch.Tensor) or timestep.dtype != res.dtype:
            raise TypeError(f"{op}: timestep must be a {res.dtype} tensor like res")
        if timestep.dim() == 2 and timestep.shape == (B, 6 * C) and timestep.stride(1) == 1:
            timestep = timestep.unflatten(1, (6, C))
        if tuple(timestep.shape) != (B, 6, C) or timestep.stride(2) != 1 or timestep.stride(1) != C:
            raise ValueError(f"{op}: timestep must be [{B}, 6, {C}] or [{B}, {6 * C}] with contiguous samples, got {tuple(timestep.shape)}")
    for name, t in (("gate_table", gate_table), ("mod_table", mod_table)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != res.dtype or tuple(t.shape) != (6, C) or not t.is_contiguous()):
            raise ValueError(f"{op}: {name} must be a contiguous {res.dtype} [6, {C}] tensor")
    for name, t in (("res", res), ("a", a), ("timestep", timestep), ("gate_table", gate_table), ("mod_table", mod_table), ("out", out), ("out_mod", out_mod)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"{op}: {name} must be a GPU tensor (there is no CPU path)")
    stats = torch.empty(B * T, 2, dtype=torch.float32, device=res.device) if want_stats else None
    ops.sana_glue(res, a, timestep, gate_table if gate_row is not None else None, mod_table if out_mod is not None else None, out, out_mod, stats,
                  T, C, C_pad, gate_row=-1 if gate_row is None else int(gate_row), scale_row=int(scale_row or 0), shift_row=int(shift_row or 0),
                  eps=eps, lds=lds)
    return out, out_mod, stats


def sandwich_norm(res: torch.Tensor, a: torch.Tensor | None = None, *, w_post: torch.Tensor | None = None, gate: torch.Tensor | None = None,
                  w_pre: torch.Tensor | None = None, scale: torch.Tensor | None = None, out: torch.Tensor | bool | None = None,
                  out_mod: torch.Tensor | bool | None = None, want_stats: bool = False, eps: float = 1e-5):
    """One pass of Z-Image's sandwich norm (``svdq_sandwich_norm``): it closes a sub-layer and opens the next.  With
    ``rms(h, w) = (h * rstd(h)) * w`` (diffusers' ``RMSNorm``; one 16-bit rounding per operation throughout, fp32 in between)::

        y = res  |  res + rms(a, w_post)  |  res + gate[b] * rms(a, w_post)            (no a | no gate | gate)
        out = y;   out_mod = rms(y, w_pre)  |  rms(y, w_pre) * scale[b]                  (no scale | scale)

    ``res`` / ``a``: ``[B, T, C]`` with unit stride on the last axis and the samples T rows apart (a column slice of a wider buffer will do);
    ``gate`` / ``scale``: ``[B, C]`` -- what the block applies: ``tanh(gate)`` and ``1 + scale``; the weights: ``[C]``.  ``out`` / ``out_mod``: a
    tensor to write into (``out`` may be ``res``), True to allocate one, None / False for none; ``out`` defaults to "when ``a`` is given",
    ``out_mod`` to "when ``w_pre`` is given".  Returns ``(out, out_mod, stats)`` with None for what was not asked for; ``stats`` is the float32
    ``[B * T, 2]`` ``(rstd(a) or 0, rstd(y))``."""
    op = "sandwich_norm"
    if not isinstance(res, torch.Tensor) or res.dim() != 3:
        raise ValueError(f"{op}: res must be a [B, T, C] tensor")
    if res.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"{op}: res must be bfloat16 or float16, got {res.dtype}")
    B, T, C = res.shape
    if C < 8 or C % 8 or B < 1 or T < 1:
        raise ValueError(f"{op}: need C={C} a multiple of 8 and at least one row, got res {tuple(res.shape)}")
    if out is None:
        out = a is not None
    if out_mod is None:
        out_mod = w_pre is not None
    out = torch.empty(B, T, C, dtype=res.dtype, device=res.device) if out is True else None if out is False else out
    out_mod = torch.empty(B, T, C, dtype=res.dtype, device=res.device) if out_mod is True else None if out_mod is False else out_mod
    if out is None and out_mod is None and not want_stats:
        raise ValueError(f"{op}: nothing to do: none of out, out_mod and stats is asked for")
    if gate is not None and a is None:
        raise ValueError(f"{op}: a gate needs a")
    if a is not None and w_post is None:
        raise ValueError(f"{op}: a needs w_post")
    if out_mod is not None and w_pre is None:
        raise ValueError(f"{op}: out_mod needs w_pre")
    if scale is not None and out_mod is None:
        raise ValueError(f"{op}: scale needs out_mod")
    if not (eps >= 0.0) or eps == float("inf"):
        raise ValueError(f"{op}: eps={eps} must be finite and not negative")

    def row_stride(name, t):
        """the row stride of a [B, T, C] view whose samples lie T rows apart (0 for None)"""
        if t is None:
            return 0
        if not isinstance(t, torch.Tensor) or t.dtype != res.dtype:
            raise TypeError(f"{op}: {name} must be a {res.dtype} tensor like res")
        if t.device != res.device:
            raise ValueError(f"{op}: {name} must live on res's device {res.device}, got {t.device}")
        if tuple(t.shape) != (B, T, C):
            raise ValueError(f"{op}: {name} must be [{B}, {T}, {C}], got {tuple(t.shape)}")
        s0, s1, s2 = t.stride()
        if s2 != 1 or (B > 1 and T > 1 and s0 != T * s1):
            raise ValueError(f"{op}: {name} must have unit stride on its last axis and hold its samples T rows apart")
        # (the strides of dimensions of size 1 are arbitrary in torch: the library gets the natural ones)
        return s1 if T > 1 else s0 if B > 1 else C

    lds = (row_stride("res", res), row_stride("a", a), row_stride("out", out), row_stride("out_mod", out_mod))
    for name, t in (("w_post", w_post), ("w_pre", w_pre)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != res.dtype or tuple(t.shape) != (C,) or not t.is_contiguous()):
            raise ValueError(f"{op}: {name} must be a contiguous {res.dtype} [{C}] tensor")
    for name, t in (("gate", gate), ("scale", scale)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != res.dtype or tuple(t.shape) != (B, C) or t.stride(1) != 1):
            raise ValueError(f"{op}: {name} must be a {res.dtype} [{B}, {C}] tensor with unit stride on its last axis")
    for name, t in (("res", res), ("a", a), ("w_post", w_post), ("gate", gate), ("w_pre", w_pre), ("scale", scale), ("out", out), ("out_mod", out_mod)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"{op}: {name} must be a GPU tensor (there is no CPU path)")
    stats = torch.empty(B * T, 2, dtype=torch.float32, device=res.device) if want_stats else None
    ops.sandwich_norm(res, a, w_post if a is not None else None, gate, w_pre if out_mod is not None else None, scale, out, out_mod, stats, T, C,
                      lds=lds, eps=eps)
    return out, out_mod, stats
