"""Operator wrappers.  The depthwise convolution and the cross-attention are exported here; every other operator is imported from its own
module."""
from .attention import cross_attention  # noqa: F401
from .conv import dwconv3x3  # noqa: F401
