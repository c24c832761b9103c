"""reference: nunchaku/caching/diffusers_adapters/flux_v2.py."""
from nunchaku_amd.caching.diffusers_adapters.flux_v2 import apply_cache_on_pipe, apply_cache_on_transformer  # noqa: F401
