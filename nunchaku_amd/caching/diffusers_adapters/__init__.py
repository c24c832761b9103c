"""Pipeline adapters of First-Block Cache (reference: nunchaku/caching/diffusers_adapters/__init__.py)."""


def apply_cache_on_pipe(pipe, *args, **kwargs):
    """Apply First-Block Cache to a pipeline, chosen by its class name as the reference does: ``Flux*`` pipelines (``flux_v2``) and
    ``QwenImage*`` pipelines (``qwenimage``; the prefix also covers the Edit pipelines' class names).

    SANA has an adapter too, but no branch here: a ``Sana*`` class name keeps raising ``Unknown pipeline class name`` from this
    dispatcher.  SANA users import ``apply_cache_on_pipe`` from ``nunchaku.caching.diffusers_adapters.sana``."""
    pipe_cls_name = pipe.__class__.__name__
    if pipe_cls_name.startswith("Flux"):
        from .flux_v2 import apply_cache_on_pipe as apply_cache_on_pipe_fn
    elif pipe_cls_name.startswith("QwenImage"):
        from .qwenimage import apply_cache_on_pipe as apply_cache_on_pipe_fn
    else:
        raise ValueError(f"Unknown pipeline class name: {pipe_cls_name}")
    return apply_cache_on_pipe_fn(pipe, *args, **kwargs)
