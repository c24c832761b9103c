"""reference: src/SanaModel.cpp:13-136 (``SanaLinearAttention``; the reference keeps its SANA layers in C++ behind transformer_sana.py)."""
from nunchaku_amd.models.sana import SanaLinearAttention, convert_sana_attention_state_dict  # noqa: F401
