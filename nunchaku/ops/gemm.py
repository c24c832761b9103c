"""reference: nunchaku/ops/gemm.py:12-160."""
from nunchaku_amd.ops.gemm import gemm_awq_multi, svdq_gemm_mxfp4, svdq_gemm_w4a4_cuda  # noqa: F401
