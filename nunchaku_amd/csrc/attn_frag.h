// Register fragments the attention kernels share (attention.hip, ip_attention.hip, cross_attention.hip, attention_d64.hip,
// linear_attention.hip): the 16-bit packing, and for the kernels on the S^T = K Q^T / O^T = V^T P^T formulation of the 32x32x16 MFMA
// (ip_attention.hip's header comment derives the operand layouts) the register-to-key map, the softmax arithmetic and its contract, the
// V transpose and the output epilogue.  A lane (lr, h) owns query row lr.
// The kernels keep what differs between them: LDS layouts and swizzles, staging loops, grids, host checks.
//
// Shape of the helpers.  hipcc optimises an always-inline function as a function of its own BEFORE it inlines it: a helper that holds a
// loop over a kernel's score or fragment array is unrolled earlier than the code around it, and the kernel's instructions then come out in
// another order with other registers.  So the helpers below are loop BODIES on scalars, or whole nests that were checked: moving a kernel
// onto them left every instantiation's code object instruction for instruction what it was (tools/isa_stats.py --diff).  The loops over
// the score tiles and P fragments stay in the kernels.
#pragma once
#include "svdq_common.h"
#include <atomic>

namespace svdq {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
// two floats -> one dword of two RNE-rounded 16-bit values (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32)
template <int DT> __device__ __forceinline__ unsigned pack2(float a, float b) {
    if constexpr (DT == SVDQ_BF16) return __builtin_bit_cast(unsigned, __builtin_convertvector((v2f){a, b}, bf16x2));
    else return __builtin_bit_cast(unsigned, __builtin_convertvector((v2f){a, b}, f16x2));
}
// the two 16-bit values of a dword, as floats
template <int DT> __device__ __forceinline__ float pk_lo(unsigned pk) { return h2f(hfrom<typename Half<DT>::T>((unsigned short)(pk & 0xffffu))); }
template <int DT> __device__ __forceinline__ float pk_hi(unsigned pk) { return h2f(hfrom<typename Half<DT>::T>((unsigned short)(pk >> 16))); }

// the key, counted from its tile's first, whose score register r of a 32-key tile holds.  The kernels set the scores of the keys at or
// beyond the count to -inf: probability exactly 0
__device__ __forceinline__ int score_key(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }

// maximum of query row lr over NKT score tiles: lane holds half of the row's scores, lane ^ 32 the other half
template <int NKT> __device__ __forceinline__ float row_max(const v16f (&s)[NKT]) {
    float m = s[0][0];
#pragma unroll
    for (int kt = 0; kt < NKT; kt++)
#pragma unroll
        for (int r = 0; r < 16; r++) m = fmaxf(m, s[kt][r]);
    return fmaxf(m, __shfl_xor(m, 32));
}

// The softmax contract of these kernels (attention.hip's), stated once:
//   * P = exp2(s c - m c) is ROUNDED to 16 bits before it meets V (prob_pair: one dword of the PV MFMA's B operand), and
//   * the row sum l is taken over those rounded values (add_rounded): l sums exactly what V is multiplied with;
//   * the normalisation by l follows the LAST MFMA (o_tile_piece).  A row dominated by one key returns that key's V row exactly.
//   * Online form, a chunk of keys at a time (online_softmax_scale): running maximum m, O and l rescaled by
//     alpha = exp2((m_old - m_new) c), which is 0 on the first chunk (m_old = -inf: nothing to keep) and 1 while the maximum stands.
// A fragment of P: the registers 8 (ks & 1) .. +7 of score tile ks / 2 are the keys of V^T piece 2 ks + h (transpose8x8_piece), two per
// dword.
template <int DT> __device__ __forceinline__ unsigned prob_pair(float s0, float s1, float c, float nmc) {
    const float e0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s0, c, nmc));
    const float e1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s1, c, nmc));
    return pack2<DT>(e0, e1);
}
template <int DT> __device__ __forceinline__ float add_rounded(float l, unsigned pk) {
    l += pk_lo<DT>(pk);
    l += pk_hi<DT>(pk);
    return l;
}
struct SoftmaxScale {
    float m, alpha, nmc; // the new running maximum; the factor for O and l; the exponent offset -(m c) for prob_pair
};
__device__ __forceinline__ SoftmaxScale online_softmax_scale(float m_run, float m_chunk, float c) {
    const float m_new = fmaxf(m_run, m_chunk);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);
    return {m_new, alpha, -(m_new * c)};
}

// V on its way to LDS, transposed.  Piece j of a V^T row holds the keys  16 (j / 2) + 4 (j % 2) + {0..3, 8..11}: the order in which the S
// accumulator delivers them (prob_pair), so P^T needs no cross-lane exchange.  rows[i]: 8 channels of the i-th of those keys;
// returns the piece of channel e of the 8
__device__ __forceinline__ v4i transpose8x8_piece(const v4i (&rows)[8], int e) {
    v4i col;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const unsigned a = (unsigned)rows[2 * w][e >> 1], b = (unsigned)rows[2 * w + 1][e >> 1];
        col[w] = (int)((e & 1) ? ((a >> 16) | (b & 0xffff0000u)) : ((a & 0xffffu) | (b << 16)));
    }
    return col;
}
// the two-channel form: v[i] = channels (c, c + 1) of the i-th key; lo / hi: the pieces of channel c / c + 1
__device__ __forceinline__ void transpose8x2_pieces(const unsigned (&v)[8], v4i &lo, v4i &hi) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const unsigned a = v[2 * w], b = v[2 * w + 1];
        lo[w] = (int)((a & 0xffffu) | (b << 16));
        hi[w] = (int)((a >> 16) | (b & 0xffff0000u));
    }
}

// round16(o * inv) of the 16 channels 16 j2 .. +15 of one O^T tile.  Lane (lr, h) holds channels 8 g + 4 h + e of the tile; a
// v_permlane32_swap per dword pair gives every lane 8 consecutive channels 16 j2 + 8 h .. +7: returns them, one 16-byte store for the
// caller, which knows whether the row and the channels exist.  (ip_attention.hip rounds twice, with out_scale in between, and keeps its
// own copy of this nest: with the transform as a functor here, its fp16 two-tile instantiation came out with other registers.)
template <int DT> __device__ __forceinline__ v4i o_tile_piece(v16f o, int j2, float inv) {
    unsigned x[2], y[2];
#pragma unroll
    for (int d2 = 0; d2 < 2; d2++) {
        float t[4];
#pragma unroll
        for (int i = 0; i < 4; i++) t[i] = o[8 * j2 + 4 * (i >> 1) + 2 * d2 + (i & 1)] * inv;
        x[d2] = pack2<DT>(t[0], t[1]);
        y[d2] = pack2<DT>(t[2], t[3]);
        const auto sw = __builtin_amdgcn_permlane32_swap(x[d2], y[d2], false, false);
        x[d2] = sw[0];
        y[d2] = sw[1];
    }
    return v4i{(int)x[0], (int)x[1], (int)y[0], (int)y[1]};
}

// Raise a kernel's limit of dynamic LDS to `bytes`, once per device: `raised` is the caller's bitmask of the devices done, one per kernel
// instantiation (callers may launch from several threads; setting the attribute twice is harmless)
inline hipError_t raise_dynamic_lds(const void *kernel, int bytes, std::atomic<unsigned long long> &raised) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 64 && (raised.load() >> dev & 1)) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && dev < 64) raised.fetch_or(1ull << dev);
    return e;
}

} // namespace svdq
