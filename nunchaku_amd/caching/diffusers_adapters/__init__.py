"""Pipeline adapters of First-Block Cache (reference: nunchaku/caching/diffusers_adapters/__init__.py)."""


def apply_cache_on_pipe(pipe, *args, **kwargs):
    """Apply First-Block Cache to a pipeline, chosen by its class name as the reference does.  Only ``Flux*`` pipelines have an
    adapter here (the reference's SANA adapter is out of scope; Qwen-Image has none in the reference either)."""
    pipe_cls_name = pipe.__class__.__name__
    if pipe_cls_name.startswith("Flux"):
        from .flux_v2 import apply_cache_on_pipe as apply_cache_on_pipe_fn
    else:
        raise ValueError(f"Unknown pipeline class name: {pipe_cls_name}")
    return apply_cache_on_pipe_fn(pipe, *args, **kwargs)
