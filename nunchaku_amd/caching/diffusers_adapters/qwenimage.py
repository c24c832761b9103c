"""First-Block Cache on the Qwen-Image transformer and its pipelines (the reference has no adapter of its own: it points to an external
library that replaces ``transformer.transformer_blocks``, which the fused engine's forward does not walk block by block).  The cached
forward itself is the model's (``NunchakuQwenImageTransformer2DModel.forward_cached``): the stages of the uncached forward with the
decision in between.

A true-CFG pipeline calls the transformer twice per step, conditional first, unconditional second, with different text lengths: the two
calls are *branches* with a set of buffers each.  Call number ``k`` of a cache context uses branch ``k % cfg_branches``."""

from __future__ import annotations

import functools
import inspect

from ..fbcache import cache_context, create_cache_context, get_current_cache_context

_CALLS = "qwenimage_transformer_calls"  # the context's counter of transformer calls


def cached_forward(self, *args, **kwargs):
    """Replaces ``transformer.forward``.  Outside a cache context the original forward runs."""
    ctx = get_current_cache_context()
    if ctx is None:
        return self._original_forward(*args, **kwargs)
    k = ctx.incremental_name_counters[_CALLS]
    ctx.incremental_name_counters[_CALLS] = k + 1
    return self.forward_cached(*args, **kwargs, residual_diff_threshold=self.residual_diff_threshold, first_blocks=self.first_blocks,
                               branch=k % max(int(self.cfg_branches), 1), verbose=getattr(self, "verbose", False))


def apply_cache_on_transformer(transformer, *, residual_diff_threshold: float = 0.12, first_blocks: int = 1, cfg_branches: int = 1):
    """Replace ``transformer.forward`` by the cached forward (once; a second call only updates the settings).  ``first_blocks``: the
    blocks that always run (1 is First-Block Cache proper; cache-dit recommends 8 for Qwen-Image).  ``cfg_branches``: transformer calls
    per denoising step (2 with true CFG)."""
    if not callable(getattr(transformer, "forward_cached", None)):
        raise TypeError(f"apply_cache_on_transformer: {type(transformer).__name__} is not a Qwen-Image transformer of this library")
    if int(cfg_branches) < 1:
        raise ValueError(f"cfg_branches must be at least 1, got {cfg_branches}")
    transformer.residual_diff_threshold = residual_diff_threshold
    transformer.first_blocks = first_blocks
    transformer.cfg_branches = int(cfg_branches)
    if getattr(transformer, "_is_cached", False):
        return transformer
    transformer._original_forward = transformer.forward
    transformer.verbose = False
    transformer.forward = cached_forward.__get__(transformer, transformer.__class__)
    transformer._is_cached = True
    return transformer


def pipeline_cfg_branches(call, args: tuple, kwargs: dict) -> int:
    """Transformer calls per step of one pipeline call, by the pipeline's own rule (diffusers ``QwenImagePipeline.__call__``:
    ``do_true_cfg = true_cfg_scale > 1 and has_neg_prompt``): 2 when ``true_cfg_scale > 1`` and a negative prompt or negative prompt
    embeddings are passed, else 1.  Arguments left out take the defaults of ``call``'s signature."""
    try:
        sig = inspect.signature(call)
        bound = sig.bind_partial(*args, **kwargs)
        bound.apply_defaults()
        given = dict(bound.arguments)
        for p in sig.parameters.values():
            if p.kind is inspect.Parameter.VAR_KEYWORD:  # a **kwargs parameter of the signature holds the rest
                given.update(given.pop(p.name, {}))
    except (TypeError, ValueError):
        given = dict(kwargs)
    scale = given.get("true_cfg_scale")
    has_negative = given.get("negative_prompt") is not None or given.get("negative_prompt_embeds") is not None
    return 2 if scale is not None and scale > 1 and has_negative else 1


def apply_cache_on_pipe(pipe, **kwargs):
    """Wrap the pipeline class's ``__call__`` (once) so that every call runs in a fresh cache context, and cache its transformer.  Unless
    ``cfg_branches`` is given, every call sets it from its own arguments (:func:`pipeline_cfg_branches`)."""
    if not getattr(pipe, "_is_cached", False):
        original_call = pipe.__class__.__call__

        @functools.wraps(original_call)
        def new_call(self, *args, **kwargs):
            transformer = getattr(self, "transformer", None)
            if getattr(transformer, "_cfg_branches_from_call", False):
                transformer.cfg_branches = pipeline_cfg_branches(original_call, (self,) + args, kwargs)
            with cache_context(create_cache_context()):
                return original_call(self, *args, **kwargs)

        pipe.__class__.__call__ = new_call
        pipe.__class__._is_cached = True

    apply_cache_on_transformer(pipe.transformer, **kwargs)
    pipe.transformer._cfg_branches_from_call = "cfg_branches" not in kwargs
    return pipe
