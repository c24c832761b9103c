"""reference: nunchaku/caching/utils_v2.py."""
from nunchaku_amd.caching.diffusers_adapters.flux_v2 import cached_forward_v2  # noqa: F401
