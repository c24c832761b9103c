"""reference: nunchaku/caching/diffusers_adapters/__init__.py."""
from nunchaku_amd.caching.diffusers_adapters import apply_cache_on_pipe  # noqa: F401
