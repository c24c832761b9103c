"""reference: nunchaku/caching/ (First-Block Cache)."""
