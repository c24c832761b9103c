// The MXFP4 block quantiser on a half-wave pair, shared by the activation quantiser (quantize_mxfp4.hip) and the GEMM's
// GELU_QUANT epilogue (gemm_mxfp4.hip).  Lane (r, h) holds 16 values of a 32-channel block of row r: pieces q = 0 .. 3, channels 8 q + 4 h + e --
// the quantiser's record layout and the order in which a 32 x 32 accumulator tile holds a row.  The rule is written out in VALU integer / fp32
// operations that are exact for every 16-bit input (a multiply by a power of two, a 1-bit mantissa rounding on the bit pattern), because a block
// of bf16 subnormals needs 2^-X = 2^127 and scales below 2^-126, which the v_cvt_scalef32_pk_fp4 converters take as fp32 scale operands.
#pragma once

#include "svdq_common.h"

namespace svdq {

// E8M0 byte of a block whose largest finite magnitude is amax (>= 0, finite): floor(log2 amax) - 2 + 127, clamped; 0 for an all-zero block
__device__ __forceinline__ unsigned mx_scale_byte(float amax) {
    const unsigned bits = __builtin_bit_cast(unsigned, amax);
    const int ef = (int)(bits >> 23);
    const int e = ef ? ef - 127 : (31 - __builtin_clz(bits | 1u)) - 149; // fp32 subnormals (the bf16 subnormals) by their leading bit
    const int sb = e + 125;
    return bits == 0u ? 0u : (unsigned)(sb < 0 ? 0 : sb > 254 ? 254 : sb);
}
// e2m1 code of y (already divided by the block scale): round to nearest, ties to the even mantissa, saturated to 6; NaN -> 0; a zero result is +0
__device__ __forceinline__ unsigned mx_code(float y) {
    const float ay = __builtin_fminf(nan_to_zero(__builtin_fabsf(y)), 6.0f);
    const unsigned lo = (unsigned)__builtin_rintf(ay * 2.0f); // below 1: the subnormal step 0.5 (0, 0.5, and 1.0 = code 2)
    unsigned u = __builtin_bit_cast(unsigned, ay);
    u += 0x1fffffu + ((u >> 22) & 1u);                         // RNE to one mantissa bit, the carry runs into the exponent
    const unsigned hi = (u >> 22) - 252u;                      // (exponent field - 127) * 2 + mantissa bit + 2
    const unsigned c = ay < 1.0f ? lo : hi;
    return c == 0u ? 0u : c | (y < 0.f ? 8u : 0u);
}
template <typename T> __device__ __forceinline__ float max_finite() {
    if constexpr (__is_same(T, _Float16)) return 65504.0f;
    else return __builtin_bit_cast(float, 0x7f7f0000u);
}

// one more value of the lane's 16 into its running amax: NaN is no part of amax
__device__ __forceinline__ float mx_amax_acc(float amax, float v) { return __builtin_fmaxf(amax, nan_to_zero(__builtin_fabsf(v))); }

// the lane's amax -> the block's scale byte: inf counts as the largest finite value, the two halves meet in one __shfl_xor
template <typename T> __device__ __forceinline__ unsigned mx_block_byte(float amax) {
    amax = __builtin_fminf(amax, max_finite<T>());
    amax = __builtin_fmaxf(amax, __shfl_xor(amax, 32));
    return mx_scale_byte(amax);
}

// the lane's 16 codes of a block with scale byte sb, from float v[16] into unsigned pc[2]: pc[t] = piece 2t | piece 2t + 1 << 16, 4 codes = 16 bits a
// piece.  A macro, not a function: behind an inlined call the compiler orders the chain of ORs by other value numbers and quantize_mxfp4_kernel
// comes out with the same instructions in another schedule (as a function: 25 s_nop fewer and commuted v_or operands); the expanded text is
// the kernel's own as it was.
#define MX_BLOCK_CODES(v, sb, pc)                                                                                                                        \
    do {                                                                                                                                                 \
        const float inv = __builtin_bit_cast(float, (254u - (sb)) << 23); /* 2^-(sb - 127), exponent field 0 .. 254: sb = 254 never occurs (amax <= 2^128) */ \
        (pc)[0] = (pc)[1] = 0;                                                                                                                           \
        _Pragma("unroll") for (int q = 0; q < 4; q++)                                                                                                    \
            _Pragma("unroll") for (int e = 0; e < 4; e++) (pc)[q >> 1] |= mx_code((v)[4 * q + e] * inv) << (16 * (q & 1) + 4 * e);                        \
    } while (0)

// the halves trade pieces of the four blocks of a 128-channel K-step: lane h keeps blocks 2h, 2h + 1 (32 contiguous bytes of the row, dw[0 .. 7]),
// dword q of a block = piece q of half 0 | piece q of half 1 << 16
__device__ __forceinline__ void mx_trade_halves(const unsigned (&pc)[4][2], int h, unsigned (&dw)[8]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned own = h ? pc[2 + (j >> 1)][j & 1] : pc[j >> 1][j & 1];
        const unsigned oth = (unsigned)__shfl_xor((int)(h ? pc[j >> 1][j & 1] : pc[2 + (j >> 1)][j & 1]), 32);
        const unsigned a = h ? oth : own, bq = h ? own : oth; // a: half 0's pieces, bq: half 1's
        dw[2 * j] = (a & 0xffffu) | (bq << 16);
        dw[2 * j + 1] = (a >> 16) | (bq & 0xffff0000u);
    }
}

} // namespace svdq
