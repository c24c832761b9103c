"""reference: nunchaku/caching/diffusers_adapters/sana.py."""
from nunchaku_amd.caching.diffusers_adapters.sana import apply_cache_on_pipe, apply_cache_on_transformer  # noqa: F401
