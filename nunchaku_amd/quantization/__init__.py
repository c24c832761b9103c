"""Host-side encoders (plain torch, not on the hot path)."""
from .mxfp4 import dequantize_mxfp4, pack_scales_mxfp4, quantize_weight_mxfp4, unpack_scales_mxfp4  # noqa: F401
