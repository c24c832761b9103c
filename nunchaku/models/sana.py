"""reference: src/SanaModel.cpp:13-136 (``SanaLinearAttention``), :138-190 (``MultiHeadCrossAttention``), :192-213 (``SanaGLUMBConv``), :215-322
(``SanaLinearTransformerBlock``) and :324-363 (``SanaModel``); the reference keeps its SANA layers in C++ behind transformer_sana.py."""
from nunchaku_amd.models.sana import (SanaCrossAttention, SanaDepthwiseConv, SanaGLUMBConv, SanaLinearAttention,  # noqa: F401
                                      SanaLinearTransformerBlock, SanaModel, convert_sana_attention_state_dict,
                                      convert_sana_cross_attention_state_dict, convert_sana_ff_state_dict, convert_sana_state_dict)
