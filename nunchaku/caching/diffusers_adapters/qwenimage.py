"""Qwen-Image adapter of First-Block Cache (the reference has none of its own)."""
from nunchaku_amd.caching.diffusers_adapters.qwenimage import apply_cache_on_pipe, apply_cache_on_transformer  # noqa: F401
