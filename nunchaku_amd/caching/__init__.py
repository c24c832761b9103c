"""Step-skipping caches (reference: nunchaku/caching/).  First-Block Cache: ``fbcache`` holds the cache context and the decision,
``utils`` the cached wrapper around SANA's stack, ``diffusers_adapters`` applies the cache to a transformer or a pipeline (FLUX,
Qwen-Image, SANA).  TeaCache (FLUX): ``teacache`` holds the context manager and the decision."""
