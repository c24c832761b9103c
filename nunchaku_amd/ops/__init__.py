"""Operator wrappers.  The depthwise convolution, the cross-attention and SANA's block glue are exported here; every other operator is
imported from its own module."""
from .attention import cross_attention  # noqa: F401
from .conv import dwconv3x3  # noqa: F401
from .elementwise import sana_glue  # noqa: F401
