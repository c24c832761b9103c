"""Operator wrappers.  The depthwise convolution is exported here; every other operator is imported from its own module."""
from .conv import dwconv3x3  # noqa: F401
