"""reference: nunchaku/caching/ (First-Block Cache, TeaCache)."""
