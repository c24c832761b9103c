// The gate activations of the split-half and interleaved GLU kernels, fp32 in and out: the tile quantisers (quantize_glu.hip,
// quantize_dwconv_glu.hip through quantize_tail.h) and the MXFP4 GEMM's GLU_QUANT epilogue (gemm_mxfp4.hip) share these expressions, so a
// gate has one value whichever kernel evaluates it.
#pragma once

#include "svdq_common.h"

namespace svdq {

// silu(g) = g * rcp(1 + exp2(-log2e g)): the form of quantize_kernel's GLU front end, bit for bit, down to g = -44.  Below, 1 + e == e in fp32 and e
// itself leaves the range at g = -88.7 although g e^g is an ordinary bf16 number down to g = -96: the exponent is carried 2^64 lower and put back
// with a multiply, which rounds into the fp32 subnormals where v_rcp_f32 would flush.
__device__ __forceinline__ float glu_silu(float g) {
    const bool big = g < -44.0f;
    const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * g - (big ? 64.0f : 0.0f));
    const float sg = g * __builtin_amdgcn_rcpf(big ? e : 1.0f + e);
    return big ? sg * 0x1p-64f : sg;
}

// gelu(g) = g * 0.5 * (1 + erf(g sqrt(1/2))) with 1 + erf(z) taken as erfc(|z|) or 2 - erfc(|z|): the same function (within 2^-23 of the
// literal form where that form is accurate), and accurate in the negative tail, where 1 + erf cancels (gelu(-6) = -6e-9 is an ordinary 16-bit number).
__device__ __forceinline__ float glu_gelu(float g) {
    const float z = g * 0.70710678118654752440f;
    const float c = erfcf(__builtin_fabsf(z));
    return g * (0.5f * (z < 0.f ? c : 2.0f - c));
}

} // namespace svdq
