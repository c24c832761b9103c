"""reference: nunchaku/caching/teacache.py."""
from nunchaku_amd.caching.teacache import TeaCache, make_teacache_forward  # noqa: F401
