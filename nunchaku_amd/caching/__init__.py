"""Step-skipping caches for the FLUX transformer (reference: nunchaku/caching/).  First-Block Cache: ``fbcache`` holds the cache context
and the decision, ``diffusers_adapters`` applies it to a transformer or a pipeline.  TeaCache: ``teacache`` holds the context manager and
the decision."""
