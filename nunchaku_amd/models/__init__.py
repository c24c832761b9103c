"""Model-side modules.  The SANA attention layer is exported here; everything else is imported from its own module."""
from .sana import SanaLinearAttention, convert_sana_attention_state_dict  # noqa: F401
