"""Operator wrappers.  The depthwise convolution, SANA's cross-attention, SDXL's head-dimension-64 attention, SANA's block glue, Z-Image's two
glue passes, PuLID's folded cross-attention, Qwen-Image's rotary-table gather and the T5 encoder's multi-weight AWQ GEMM and residual norm are
exported here; every other operator is imported from its own module."""
from .attention import attention_d64, attention_d64_bias, cross_attention, pulid_ca, qk_norm_rope  # noqa: F401
from .conv import dwconv3x3  # noqa: F401
from .elementwise import sana_glue, sandwich_norm, t5_residual_norm  # noqa: F401
from .gemm import gemm_awq_multi, svdq_gemm_mxfp4  # noqa: F401
from .quantize import svdq_quantize_dwconv_glu, svdq_quantize_glu_halves, svdq_quantize_mxfp4  # noqa: F401
from .rotary import qwen_rotary  # noqa: F401
