"""First-Block Cache: context, buffers and the decision (reference: nunchaku/caching/fbcache.py, adapted there from ParaAttention).

After the first transformer block of a denoising step the change that block made to the image stream (its *first residual*) is
compared with the first residual of the last fully computed step.  If the relative L1 distance is below the threshold the other
blocks are skipped and their summed effect at that step (``multi_hidden_states_residual`` ...) is added instead; otherwise they run
and the buffers are replaced.  Names, arguments, buffer names and semantics are the reference's.  Two of them are easy to get wrong:

* on a **hit the stored first residual is not replaced**: a run of hits keeps comparing against the last computed step;
* with no stored first residual the answer is "miss" (and the reported distance is the threshold).

On GPU 16-bit tensors :func:`are_two_tensors_similar` is one pass of ``svdq_residual_diff`` (the reference runs six torch launches)
with the reference's rounding points; the decision is taken from the 16-bit means and their 16-bit quotient, as torch takes it.
Reading the result synchronises the stream.
"""

from __future__ import annotations

import contextlib
import dataclasses
from collections import defaultdict
from typing import DefaultDict, Dict, Optional, Tuple

import torch


@dataclasses.dataclass
class CacheContext:
    """Named tensor buffers of one generation (one pipeline call) and counters for incremental names."""

    buffers: Dict[str, torch.Tensor] = dataclasses.field(default_factory=dict)
    incremental_name_counters: DefaultDict[str, int] = dataclasses.field(default_factory=lambda: defaultdict(int))

    def get_incremental_name(self, name=None):
        if name is None:
            name = "default"
        idx = self.incremental_name_counters[name]
        self.incremental_name_counters[name] += 1
        return f"{name}_{idx}"

    def reset_incremental_name(self):
        self.incremental_name_counters.clear()

    def get_buffer(self, name: str) -> Optional[torch.Tensor]:
        return self.buffers.get(name)

    def set_buffer(self, name: str, buffer: torch.Tensor):
        self.buffers[name] = buffer

    def clear_buffers(self):
        self.buffers.clear()


_current_cache_context = None


def create_cache_context() -> CacheContext:
    return CacheContext()


def get_current_cache_context():
    return _current_cache_context


@contextlib.contextmanager
def cache_context(cache_context):
    """Make ``cache_context`` the active one inside the ``with`` block; the previous one comes back on exit."""
    global _current_cache_context
    old_cache_context = _current_cache_context
    _current_cache_context = cache_context
    try:
        yield
    finally:
        _current_cache_context = old_cache_context


def get_buffer(name: str) -> Optional[torch.Tensor]:
    cache_context = get_current_cache_context()
    assert cache_context is not None, "cache_context must be set before"
    return cache_context.get_buffer(name)


def set_buffer(name: str, buffer: torch.Tensor):
    cache_context = get_current_cache_context()
    assert cache_context is not None, "cache_context must be set before"
    cache_context.set_buffer(name, buffer)


def attach_comparison(first_residual: torch.Tensor, prev: torch.Tensor, record) -> torch.Tensor:
    """The engine subtracts and compares in ONE launch (``ops.elementwise.residual_diff`` with a base and the stored residual): it hands
    the pending result over with the residual, and :func:`are_two_tensors_similar` on exactly this pair reads it instead of launching again."""
    first_residual._fbcache_compared = (prev, record)
    return first_residual


def are_two_tensors_similar(t1: torch.Tensor, t2: torch.Tensor, *, threshold: float, parallelized: bool = False):
    """``mean(|t1 - t2|) / mean(|t1|) < threshold`` -> ``(is_similar, diff_ratio)`` as 0-dim tensors.  ``parallelized`` is unused, as
    in the reference.  GPU bf16 / fp16 tensors go through the ``svdq_residual_diff`` kernel (the result is read on the host: 0-dim CPU
    tensors come back, and a stream under capture raises); every other tensor (CPU, fp32) takes the reference's torch ops."""
    compared = t2.__dict__.pop("_fbcache_compared", None)
    if compared is not None and compared[0] is t1:
        record = compared[1]
    elif t1.is_cuda and t2.is_cuda and t1.dtype == t2.dtype and t1.dtype in (torch.bfloat16, torch.float16):
        from ..ops.elementwise import residual_diff

        if t1.shape != t2.shape:
            raise ValueError(f"are_two_tensors_similar: shapes differ: {tuple(t1.shape)} vs {tuple(t2.shape)}")
        record = residual_diff(t2.contiguous(), prev=t1.contiguous())[1]
    else:
        mean_diff = (t1 - t2).abs().mean()
        mean_t1 = t1.abs().mean()
        diff_ratio = mean_diff / mean_t1
        return diff_ratio < threshold, diff_ratio
    return record.is_similar(threshold), record.ratio


def apply_prev_hidden_states_residual(hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor | None = None,
                                      mode: str = "multi", suffix: str = "") -> Tuple[torch.Tensor, torch.Tensor]:
    """Add the stored residuals of the skipped blocks: ``(hidden, encoder_hidden)`` for ``mode="multi"``, ``hidden`` for ``"single"``.
    ``suffix`` (extension): appended to the buffer names."""
    if mode == "multi":
        hidden_states_residual = get_buffer("multi_hidden_states_residual" + suffix)
        assert hidden_states_residual is not None, "multi_hidden_states_residual must be set before"
        hidden_states = (hidden_states + hidden_states_residual).contiguous()
        if encoder_hidden_states is not None:
            enc_hidden_res = get_buffer("multi_encoder_hidden_states_residual" + suffix)
            assert enc_hidden_res is not None, "multi_encoder_hidden_states_residual must be set before"
            encoder_hidden_states = (encoder_hidden_states + enc_hidden_res).contiguous()
        return hidden_states, encoder_hidden_states
    elif mode == "single":
        single_residual = get_buffer("single_hidden_states_residual" + suffix)
        assert single_residual is not None, "single_hidden_states_residual must be set before"
        return (hidden_states + single_residual).contiguous()
    raise ValueError(f"Unknown mode {mode}; expected 'multi' or 'single'")


def _first_name(mode: str) -> str:
    if mode == "multi":
        return "first_multi_hidden_states_residual"
    if mode == "single":
        return "first_single_hidden_states_residual"
    raise ValueError(f"Unknown mode {mode}; expected 'multi' or 'single'")


def get_can_use_cache(first_hidden_states_residual: torch.Tensor, threshold: float, parallelized: bool = False, mode: str = "multi",
                      suffix: str = ""):
    """``(can_use_cache, diff)``: the stored first residual of ``mode`` against the current one; no stored residual: ``(False, threshold)``.
    ``suffix`` (extension): appended to the buffer name -- one set of buffers per branch of a true-CFG step."""
    prev_res = get_buffer(_first_name(mode) + suffix)
    if prev_res is None:
        first_hidden_states_residual.__dict__.pop("_fbcache_compared", None)
        return torch.tensor(False), torch.tensor(threshold)
    return are_two_tensors_similar(prev_res, first_hidden_states_residual, threshold=threshold, parallelized=parallelized)


def check_and_apply_cache(*, first_residual: torch.Tensor, hidden_states: torch.Tensor,
                          encoder_hidden_states: Optional[torch.Tensor] = None, threshold: float, parallelized: bool, mode: str,
                          verbose: bool, call_remaining_fn, remaining_kwargs,
                          apply_residual_fn=None, suffix: str = "") -> Tuple[torch.Tensor, Optional[torch.Tensor], float]:
    """The state machine of a cached step.  Hit: the stored residuals are added (the stored FIRST residual stays).  Miss: ``first_residual``
    is stored, ``call_remaining_fn(hidden_states=..., encoder_hidden_states=..., **remaining_kwargs)`` runs the other blocks and returns
    ``(hidden, encoder_hidden, hidden_residual, encoder_residual)`` (``"multi"``) or ``(hidden, residual)`` (``"single"``), which are stored.
    Returns ``(hidden, encoder_hidden or None, threshold)``.  ``apply_residual_fn(hidden_states, encoder_hidden_states, mode)`` (extension)
    replaces :func:`apply_prev_hidden_states_residual` on a hit: the engine adds the residuals with its fused pass.  ``suffix`` (extension)
    is appended to every buffer name (an ``apply_residual_fn`` reads the same names).  A ``"multi"`` step that hands in no text
    stream and gets no text residual back stores none."""
    can_use_cache, diff = get_can_use_cache(first_residual, threshold=threshold, parallelized=parallelized, mode=mode, suffix=suffix)

    if can_use_cache:
        if verbose:
            diff_val = diff.item() if isinstance(diff, torch.Tensor) else diff
            print(f"[{mode.upper()}] Cache hit! diff={diff_val:.4f}, new threshold={threshold:.4f}")
        if apply_residual_fn is not None:
            out = apply_residual_fn(hidden_states, encoder_hidden_states, mode=mode)
        else:
            out = apply_prev_hidden_states_residual(hidden_states, encoder_hidden_states, mode=mode, suffix=suffix)
        updated_h, updated_enc = out if isinstance(out, tuple) else (out, None)
        return updated_h, updated_enc, threshold

    if verbose:
        diff_val = diff.item() if isinstance(diff, torch.Tensor) else diff
        print(f"[{mode.upper()}] Cache miss. diff={diff_val:.4f}, was={threshold:.4f} => now={threshold:.4f}")

    set_buffer(_first_name(mode) + suffix, first_residual)
    result = call_remaining_fn(hidden_states=hidden_states, encoder_hidden_states=encoder_hidden_states, **remaining_kwargs)

    if mode == "multi":
        updated_h, updated_enc, hs_res, enc_res = result
        set_buffer("multi_hidden_states_residual" + suffix, hs_res)
        if enc_res is not None or encoder_hidden_states is not None:
            set_buffer("multi_encoder_hidden_states_residual" + suffix, enc_res)
        return updated_h, updated_enc, threshold
    updated_cat_states, cat_res = result
    set_buffer("single_hidden_states_residual" + suffix, cat_res)
    return updated_cat_states, None, threshold
