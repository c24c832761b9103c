"""Model-side modules.  The SANA layers, block and stack are exported here; everything else is imported from its own module."""
from .sana import (SanaCrossAttention, SanaDepthwiseConv, SanaGLUMBConv, SanaLinearAttention, SanaLinearTransformerBlock, SanaModel,  # noqa: F401
                   convert_sana_attention_state_dict, convert_sana_cross_attention_state_dict, convert_sana_ff_state_dict, convert_sana_state_dict,
                   sana_intermediate_size)
