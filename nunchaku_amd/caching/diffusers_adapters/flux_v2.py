"""First-Block Cache on the FLUX transformer and its pipeline (reference: nunchaku/caching/diffusers_adapters/flux_v2.py,
caching/utils_v2.py).  The cached forward itself is the engine's (``FluxEngineMixin.engine_forward_cached``): the same stages as the
uncached forward with the decision in between."""

from __future__ import annotations

import functools

from ...models.flux import FluxEngineMixin
from ..fbcache import cache_context, create_cache_context


def cached_forward_v2(self, hidden_states, encoder_hidden_states=None, pooled_projections=None, timestep=None, img_ids=None,
                      txt_ids=None, guidance=None, joint_attention_kwargs=None, controlnet_block_samples=None,
                      controlnet_single_block_samples=None, return_dict: bool = True, controlnet_blocks_repeat: bool = False):
    """Replaces ``transformer.forward``.  A negative ``residual_diff_threshold_multi`` runs the original forward.  Otherwise: batch 1
    only, no ControlNet residuals (both raise -- the reference's cached forward drops the residuals silently), not under stream
    capture (the decision is read on the host); needs an active ``cache_context``."""
    if self.residual_diff_threshold_multi < 0.0:
        return self._original_forward(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance,
                                      **_extra_kwargs(self, joint_attention_kwargs, controlnet_block_samples,
                                                      controlnet_single_block_samples, return_dict, controlnet_blocks_repeat))
    if txt_ids is not None and txt_ids.ndim == 3:
        txt_ids = txt_ids[0]
    if img_ids is not None and img_ids.ndim == 3:
        img_ids = img_ids[0]
    out = self.engine_forward_cached(hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance,
                                     controlnet_block_samples, controlnet_single_block_samples,
                                     use_double_fb_cache=self.use_double_fb_cache,
                                     residual_diff_threshold_multi=self.residual_diff_threshold_multi,
                                     residual_diff_threshold_single=self.residual_diff_threshold_single,
                                     verbose=getattr(self, "verbose", False),
                                     ip_hidden_states=(joint_attention_kwargs or {}).get("ip_hidden_states"))
    if not _pipeline_signature(self):
        return out
    from ...models.transformer_flux import Transformer2DModelOutput

    return Transformer2DModelOutput(sample=out) if return_dict else (out,)


def _pipeline_signature(transformer) -> bool:
    """the diffusers-facing class takes the pipeline's keywords and returns an output object; the stand-alone model returns the tensor"""
    from ...models.flux import FluxTransformerAMD

    return not isinstance(transformer, FluxTransformerAMD)


def _extra_kwargs(transformer, joint_attention_kwargs, cbs, csbs, return_dict, repeat) -> dict:
    if not _pipeline_signature(transformer):
        if cbs is not None or csbs is not None:
            raise ValueError("FluxTransformerAMD.forward takes no ControlNet residuals")
        return {}
    return dict(joint_attention_kwargs=joint_attention_kwargs, controlnet_block_samples=cbs, controlnet_single_block_samples=csbs,
                return_dict=return_dict, controlnet_blocks_repeat=repeat)


def apply_cache_on_transformer(transformer, *, use_double_fb_cache: bool = False, residual_diff_threshold: float = 0.12,
                               residual_diff_threshold_multi: float | None = None, residual_diff_threshold_single: float | None = None):
    """Replace ``transformer.forward`` by the cached forward (once; a second call only updates the thresholds and the mode).
    ``transformer``: ``NunchakuFluxTransformer2DModelV2`` or the stand-alone ``FluxTransformerAMD``.  ``residual_diff_threshold_multi``
    defaults to ``residual_diff_threshold``; ``residual_diff_threshold_single`` is used with ``use_double_fb_cache`` (second decision
    behind the first single block)."""
    if not isinstance(transformer, FluxEngineMixin):
        raise TypeError(f"apply_cache_on_transformer: {type(transformer).__name__} is not a FLUX transformer of this library")
    if residual_diff_threshold_multi is None:
        residual_diff_threshold_multi = residual_diff_threshold

    if getattr(transformer, "_is_cached", False):
        transformer.residual_diff_threshold_multi = residual_diff_threshold_multi
        transformer.residual_diff_threshold_single = residual_diff_threshold_single
        transformer.use_double_fb_cache = use_double_fb_cache
        return transformer

    transformer._original_forward = transformer.forward
    transformer.residual_diff_threshold_multi = residual_diff_threshold_multi
    transformer.residual_diff_threshold_single = residual_diff_threshold_single if residual_diff_threshold_single is not None else -1.0
    transformer.use_double_fb_cache = use_double_fb_cache
    transformer.verbose = False
    transformer.forward = cached_forward_v2.__get__(transformer, transformer.__class__)
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
