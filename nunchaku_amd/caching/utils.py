"""First-Block Cache around SANA's quantised stack (reference: nunchaku/caching/utils.py ``SanaCachedTransformerBlocks``).

diffusers' ``SanaTransformer2DModel.forward`` walks ``transformer_blocks`` and calls each entry with its per-block argument list; this
library's model holds ONE entry, the whole stack (``NunchakuSanaTransformerBlocks``).  The cached wrapper takes that entry's place for a
forward: block 0 alone (``forward_layer_at(0, ...)``), the decision, then either the stored residual or the other blocks
(``forward(..., skip_first_layer=True)``).

Row convention: the first residual is ONE problem over all ``B * T`` rows -- the reference's means run over the whole ``[B, T, dim]``
tensor, so the two samples of a CFG batch take one decision together.

The subtraction, the comparison and the add run on the stack's device in the stack's dtype: the wrapper casts and moves the stream once
on the way in and once on the way out (where ``NunchakuSanaTransformerBlocks._call`` would do it around every call), so that on the
GPU the residual is formed and compared in one ``svdq_residual_diff`` pass and a hit is one ``svdq_residual_gate_stats`` add; only the
decision is read on the host.  Everything else (CPU tensors, fp32) takes the reference's torch ops."""

from __future__ import annotations

import logging

import torch
from torch import nn

from .fbcache import (apply_prev_hidden_states_residual, are_two_tensors_similar, attach_comparison, cache_context,  # noqa: F401
                      check_and_apply_cache, create_cache_context, get_buffer, get_can_use_cache, get_current_cache_context, set_buffer)

logger = logging.getLogger(__name__)

FIRST_RESIDUAL, STACK_RESIDUAL = "first_multi_hidden_states_residual", "multi_hidden_states_residual"


def _on_kernel(*tensors) -> bool:
    """16-bit GPU tensors of one dtype: the fused passes take them"""
    t0 = tensors[0]
    return all(t.is_cuda and t.dtype == t0.dtype and t.device == t0.device for t in tensors) and t0.dtype in (torch.bfloat16, torch.float16)


def _same_layout(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and a.device == b.device


def _subtract(cur: torch.Tensor, base: torch.Tensor, prev_name: str | None = None) -> torch.Tensor:
    """``cur - base`` and -- with ``prev_name``, in the same launch on the GPU -- its distance to the stored tensor of that name, handed to
    ``are_two_tensors_similar`` with the result.  A stored tensor of another shape, dtype or device is dropped: as good as not stored."""
    prev = get_buffer(prev_name) if prev_name is not None else None
    if prev is not None and not _same_layout(prev, cur):
        get_current_cache_context().buffers.pop(prev_name)
        prev = None
    if not _on_kernel(cur, base):
        return cur - base
    from ..ops.elementwise import residual_diff

    usable = prev is not None and prev.is_contiguous()
    res, record = residual_diff(cur, base, prev if usable else None)
    return attach_comparison(res, prev, record) if usable else res


class SanaCachedTransformerBlocks(nn.Module):
    """Stands where ``transformer.transformer_blocks[0]`` stands and is called with diffusers' per-block argument list.

    ``residual_diff_threshold <= 0`` or a batch above 2 (3 is what perturbed-attention guidance produces) runs the uncached stack.
    Otherwise: block 0, ``first = after - before`` over all ``B * T`` rows, the decision of ``fbcache.check_and_apply_cache`` against the
    stored ``first_multi_hidden_states_residual``; hit: ``after + multi_hidden_states_residual``; miss: the other blocks, and
    ``multi_hidden_states_residual = final - after`` is stored.  Needs an active ``cache_context`` on the cached path."""

    def __init__(self, *, transformer=None, residual_diff_threshold, verbose: bool = False):
        super().__init__()
        # not a registered child: while the adapter has this wrapper in the transformer's place the module tree would contain itself
        object.__setattr__(self, "transformer", transformer)
        self.transformer_blocks = transformer.transformer_blocks
        self.residual_diff_threshold = residual_diff_threshold
        self.verbose = verbose
        self._told_batch = False

    def forward(self, hidden_states, attention_mask, encoder_hidden_states, encoder_attention_mask=None, timestep=None,
                post_patch_height=None, post_patch_width=None):
        stack = self.transformer_blocks[0]
        kw = dict(attention_mask=attention_mask, encoder_hidden_states=encoder_hidden_states, encoder_attention_mask=encoder_attention_mask,
                  timestep=timestep, height=post_patch_height, width=post_patch_width)
        batch = hidden_states.shape[0]
        if self.residual_diff_threshold <= 0.0 or batch > 2:
            if batch > 2 and not self._told_batch:
                logger.info("SANA First-Block Cache: batch %d > 2 is not cached (CFG batches of 1 or 2 are); the uncached stack runs", batch)
                self._told_batch = True
            return stack(hidden_states=hidden_states, skip_first_layer=False, **kw)

        out_dtype, out_device = hidden_states.dtype, hidden_states.device
        dtype, device = getattr(stack, "dtype", None), getattr(stack, "device", None)
        if isinstance(dtype, torch.dtype) and device is not None:  # once, here: the stack's own casts around every call become no-ops
            hidden_states = hidden_states.to(dtype).to(device)
        before = hidden_states.contiguous()
        after = stack.forward_layer_at(0, hidden_states=before, **kw).contiguous()
        first = _subtract(after, before, FIRST_RESIDUAL)
        del before

        def apply_residual(hidden_states, encoder_hidden_states, mode):
            res = get_buffer(STACK_RESIDUAL)
            assert res is not None, f"{STACK_RESIDUAL} must be set before"
            if _on_kernel(hidden_states, res) and _same_layout(hidden_states, res) and res.is_contiguous():
                from ..ops.elementwise import residual_gate_stats

                return residual_gate_stats(hidden_states, res, want_stats=False)[0], None  # one 16-bit add, in place
            return (hidden_states + res).contiguous(), None

        def remaining(hidden_states, encoder_hidden_states):
            final = stack(hidden_states=hidden_states, skip_first_layer=True, **kw).contiguous()
            return final, None, _subtract(final, hidden_states), None

        out, _, _ = check_and_apply_cache(
            first_residual=first, hidden_states=after, encoder_hidden_states=None, threshold=self.residual_diff_threshold,
            parallelized=False, mode="multi", verbose=self.verbose, call_remaining_fn=remaining, remaining_kwargs={},
            apply_residual_fn=apply_residual)
        return out.to(out_dtype).to(out_device)
