"""reference: src/SanaModel.cpp:13-136 (``SanaLinearAttention``) and :192-213 (``SanaGLUMBConv``); the reference keeps its SANA layers in C++ behind
transformer_sana.py."""
from nunchaku_amd.models.sana import (SanaDepthwiseConv, SanaGLUMBConv, SanaLinearAttention, convert_sana_attention_state_dict,  # noqa: F401
                                      convert_sana_ff_state_dict)
