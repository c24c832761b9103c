"""First-Block Cache on the SANA transformer and its pipeline (reference: nunchaku/caching/diffusers_adapters/sana.py).

SANA users import from here (``nunchaku.caching.diffusers_adapters.sana``): the top-level dispatcher has no SANA branch."""

from __future__ import annotations

import functools

from ..fbcache import cache_context, create_cache_context, get_current_cache_context
from ..utils import SanaCachedTransformerBlocks


def apply_cache_on_transformer(transformer, *, residual_diff_threshold: float = 0.12, verbose: bool = False):
    """Wrap ``transformer.forward`` (once; a second call only updates the settings): a forward made inside a ``cache_context`` runs with
    ``transformer.transformer_blocks`` replaced by ``[SanaCachedTransformerBlocks]`` and gets the list back afterwards, whatever happens
    (the reference patches the attribute with ``unittest.mock`` for the same effect); outside a context the original forward runs."""
    if getattr(transformer, "_is_cached", False):
        cached = transformer._cached_transformer_blocks[0]
        cached.residual_diff_threshold, cached.verbose = residual_diff_threshold, verbose
        return transformer

    blocks = transformer.transformer_blocks
    cached = type(blocks)([SanaCachedTransformerBlocks(transformer=transformer, residual_diff_threshold=residual_diff_threshold, verbose=verbose)])
    original_forward = transformer.forward

    @functools.wraps(original_forward)
    def new_forward(self, *args, **kwargs):
        if get_current_cache_context() is None:
            return original_forward(*args, **kwargs)
        original_blocks = self.transformer_blocks
        self.transformer_blocks = cached
        try:
            return original_forward(*args, **kwargs)
        finally:
            self.transformer_blocks = original_blocks

    object.__setattr__(transformer, "_cached_transformer_blocks", cached)  # (not a registered child of an nn.Module: it holds the same stack)
    transformer.forward = new_forward.__get__(transformer)
    transformer._is_cached = True
    return transformer


def apply_cache_on_pipe(pipe, **kwargs):
    """Wrap the pipeline class's ``__call__`` so that every call runs in a fresh cache context, and cache its transformer."""
    if not getattr(pipe, "_is_cached", False):
        original_call = pipe.__class__.__call__

        @functools.wraps(original_call)
        def new_call(self, *args, **kwargs):
            with cache_context(create_cache_context()):
                return original_call(self, *args, **kwargs)

        pipe.__class__.__call__ = new_call
        pipe.__class__._is_cached = True

    apply_cache_on_transformer(pipe.transformer, **kwargs)
    return pipe
