"""reference: nunchaku/caching/utils.py."""
from nunchaku_amd.caching.utils import (SanaCachedTransformerBlocks, apply_prev_hidden_states_residual, are_two_tensors_similar,  # noqa: F401
                                        cache_context, create_cache_context, get_buffer, get_can_use_cache,
                                        get_current_cache_context, set_buffer)
