"""reference: nunchaku/models/ip_adapter/diffusers_adapters/__init__.py."""


def apply_IPA_on_pipe(pipe, *args, **kwargs):
    """Attach an IP-Adapter to a FLUX pipeline's transformer (``repo_id``: local file, directory, state dict or hub id)."""
    name = pipe.__class__.__name__
    if not (name.startswith("Flux") or name.startswith("IPAFlux")):
        raise ValueError(f"Unknown pipeline class name: {name}")
    from .flux import apply_IPA_on_pipe as apply_IPA_on_pipe_fn

    return apply_IPA_on_pipe_fn(pipe, *args, **kwargs)
