"""Operator wrappers.  The depthwise convolution, SANA's cross-attention, SDXL's head-dimension-64 attention and SANA's block glue are exported here; every other operator is
imported from its own module."""
from .attention import attention_d64, cross_attention  # noqa: F401
from .conv import dwconv3x3  # noqa: F401
from .elementwise import sana_glue  # noqa: F401
