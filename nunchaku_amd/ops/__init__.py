"""Operator wrappers.  The depthwise convolution, SANA's cross-attention, SDXL's head-dimension-64 attention, SANA's block glue, Z-Image's two
glue passes, PuLID's folded cross-attention and Qwen-Image's rotary-table gather are exported here; every other operator is imported from
its own module."""
from .attention import attention_d64, cross_attention, pulid_ca, qk_norm_rope  # noqa: F401
from .conv import dwconv3x3  # noqa: F401
from .elementwise import sana_glue, sandwich_norm  # noqa: F401
from .rotary import qwen_rotary  # noqa: F401
