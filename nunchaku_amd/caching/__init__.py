"""First-Block Cache for the FLUX transformer (reference: nunchaku/caching/): ``fbcache`` holds the cache context and the
decision, ``diffusers_adapters`` applies it to a transformer or a pipeline."""
