// svdq_qk_norm_rope: what stands between Z-Image's QKV projection and its attention (reference: NunchakuZSingleStreamAttnProcessor,
// nunchaku/models/attention_processors/zimage.py:35-88 -- two per-head RMSNorms, a RoPE through fp32 complex tensors and three
// unflatten / transpose copies into SDPA).  One launch per sample rewrites the Q and K thirds of the packed [T, 3 * H * 128] projection in
// place and writes V transposed, which is what svdq_attention reads:
//
//   n = rms(q, norm_q) = round16(round16(q * rstd(q)) * norm_q),   rstd(q) = 1 / sqrt(mean_128(q^2) + eps)       (norm NULL: n = q)
//   q'[2i] = round16(n[2i] * c - n[2i+1] * s),  q'[2i+1] = round16(n[2i] * s + n[2i+1] * c),  (c, s) = freqs[t, i] (freqs NULL: q' = n)
//   vt[h * 128 + d, t] = v[t, h * 128 + d] for t < T, +0 for T <= t < L_pad
//
// Plain fp32 multiplies and adds between the roundings, no contraction (see sandwich_norm.hip for op32).
//
// A workgroup takes 64 tokens of one head.  Q and K: a row of 128 values is 16 lanes x one 16-byte piece, a wave instruction covers four
// rows (256 contiguous bytes each); a lane adds the squares of its eight values in index order, a 4-level butterfly folds the 16 lanes.  The
// rotation pairs (2i, 2i + 1) lie inside a piece, and the lane's four (c, s) pairs are 32 contiguous bytes of freqs.  V: the 64 x 128 tile
// goes through 16 KiB of LDS.  It is written as read from memory, one 16-byte piece per lane, with the piece index XOR-ed by the token's
// octet ((t >> 3) & 7): the transposed read -- a lane gathers eight consecutive tokens of one channel, the eight lanes of a channel cover
// the eight octets -- then finds the eight octets in eight different piece slots = 32 different banks, without padding; its eight values
// are one 16-byte store, eight lanes write the 128 contiguous bytes of a V^T row.  No atomics.
#include <cmath>

#include "row_pass.h"

namespace svdq {

template <typename T> __device__ __forceinline__ float qk_op32(float v) {
    if constexpr (__is_same(T, _Float16)) asm("" : "+v"(v));
    return v;
}
template <typename T> __device__ __forceinline__ float qk_round(float v) { return round16<T>(qk_op32<T>(v)); }

constexpr int QK_D = 128, QK_TOK = 64;

template <int DT>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(uint16_t *qkv, const uint16_t *__restrict__ norm_q, const uint16_t *__restrict__ norm_k,
                                                           const float *__restrict__ freqs, uint16_t *__restrict__ vt, float *__restrict__ rstd_out,
                                                           int ld, int ldvt, int T, int L_pad, int H, float eps) {
    using T16 = typename Half<DT>::T;
    __shared__ u16x8 tile[QK_TOK * (QK_D / 8)]; // [token][piece ^ octet(token)]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t0 = blockIdx.x * QK_TOK, h = blockIdx.y;
    const int HD = H * QK_D;
    const int piece = lane & 15, sub = lane >> 4;
    const u16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    if (t0 < T) {
        // ---- Q and K: 128 row tasks (64 tokens x {Q, K}), four per wave instruction
#pragma unroll 1
        for (int it = 0; it < 8; it++) {
            const int task = it * 16 + wave * 4 + sub;
            const int which = task >> 6; // 0 = Q, 1 = K (wave-uniform: it >> 2)
            const int t = t0 + (task & 63);
            const uint16_t *w = which ? norm_k : norm_q;
            if (!w && !freqs) continue; // (wave-uniform) nothing to rewrite
            const bool live = t < T;    // (uniform over the 16 lanes of a row)
            uint16_t *p = qkv + (size_t)(live ? t : 0) * ld + (size_t)which * HD + h * QK_D + piece * 8;
            const u16x8 xv = live ? ld8(p) : zero;
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; e++) x[e] = h2f(hfrom<T16>(xv[e]));
            float r = 0.f;
            if (w) {
                float sq = 0.f;
#pragma unroll
                for (int e = 0; e < 8; e++) sq = sq + x[e] * x[e];
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
                r = 1.0f / sqrtf(sq / (float)QK_D + eps);
                const u16x8 wv = ld8(w + piece * 8);
#pragma unroll
                for (int e = 0; e < 8; e++) x[e] = qk_round<T16>(qk_round<T16>(x[e] * r) * h2f(hfrom<T16>(wv[e])));
            }
            if (!live) continue;
            if (rstd_out && piece == 0) rstd_out[(size_t)t * (2 * H) + which * H + h] = r;
            u16x8 ov;
            if (freqs) {
                const v4f *f = reinterpret_cast<const v4f *>(freqs + ((size_t)t * (QK_D / 2) + piece * 4) * 2);
                const v4f f0 = f[0], f1 = f[1]; // (c, s) of pairs 0, 1 and 2, 3
                const float cs[8] = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float c = cs[2 * j], s = cs[2 * j + 1], n0 = x[2 * j], n1 = x[2 * j + 1];
                    const float p0 = n0 * c, p1 = n1 * s, p2 = n0 * s, p3 = n1 * c;
                    ov[2 * j] = hbits(f2h<T16>(qk_op32<T16>(p0 - p1)));
                    ov[2 * j + 1] = hbits(f2h<T16>(qk_op32<T16>(p2 + p3)));
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; e++) ov[e] = hbits(f2h<T16>(x[e]));
            }
            st8(p, ov);
        }
    }
    if (!vt) return; // (uniform)
    // ---- V: 64 rows of 16 pieces in, 128 rows of 64 tokens out
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int tt = it * 16 + wave * 4 + sub, t = t0 + tt;
        const u16x8 vv = t < T ? ld8(qkv + (size_t)t * ld + 2 * (size_t)HD + h * QK_D + piece * 8) : zero;
        tile[tt * 16 + (piece ^ ((tt >> 3) & 7))] = vv;
    }
    __syncthreads();
    const uint16_t *tile16 = reinterpret_cast<const uint16_t *>(tile);
    const int oct = lane & 7, dr = lane >> 3;
    if (t0 + oct * 8 >= L_pad) return; // (L_pad % 8 == 0: an octet lies on one side of it) nothing is written beyond L_pad
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int dg = wave * 4 + it; // the channels dg * 8 .. + 7 = piece dg of a row
        u16x8 ov;
#pragma unroll
        for (int j = 0; j < 8; j++) ov[j] = tile16[((oct * 8 + j) * 16 + (dg ^ oct)) * 8 + dr];
        st8(vt + (size_t)(h * QK_D + dg * 8 + dr) * ldvt + t0 + oct * 8, ov);
    }
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_qk_norm_rope(const svdq_qk_norm_rope_args *a, void *stream) {
    const char *op = "svdq_qk_norm_rope";
    if (!a) { set_error("%s: args is NULL", op); return SVDQ_E_INVALID; }
    if (!a->qkv) { set_error("%s: qkv is required", op); return SVDQ_E_INVALID; }
    if (a->T < 1 || a->H < 1 || a->H > 65535) { set_error("%s: need T=%d >= 1 and 1 <= H=%d <= 65535", op, a->T, a->H); return SVDQ_E_INVALID; }
    if (a->head_dim != QK_D) { set_error("%s: head_dim=%d: 128 is implemented", op, a->head_dim); return SVDQ_E_UNSUPPORTED; }
    const long long width = 3LL * a->H * QK_D;
    if (a->ld < width || a->ld % 8) { set_error("%s: ld=%d must be at least 3 * H * 128 = %lld and a multiple of 8", op, a->ld, width); return SVDQ_E_INVALID; }
    if (a->vt) {
        if (a->L_pad < a->T || a->L_pad % 128) { set_error("%s: L_pad=%d must be at least T=%d and a multiple of 128", op, a->L_pad, a->T); return SVDQ_E_INVALID; }
        if (a->ldvt < a->L_pad || a->ldvt % 8) { set_error("%s: ldvt=%d must be at least L_pad=%d and a multiple of 8", op, a->ldvt, a->L_pad); return SVDQ_E_INVALID; }
    }
    if (!aligned_to(16, {a->qkv, a->norm_q, a->norm_k, a->vt}) || !aligned_to(16, {a->freqs}) || !aligned_to(4, {a->rstd})) {
        set_error("%s: qkv, norm_q, norm_k, vt and freqs must be 16-byte aligned, rstd 4-byte aligned", op);
        return SVDQ_E_INVALID;
    }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("%s: unknown dtype %d", op, a->dtype); return SVDQ_E_INVALID; }
    if (!(a->eps >= 0.f) || !std::isfinite(a->eps)) { set_error("%s: eps must be finite and not negative", op); return SVDQ_E_INVALID; }
    const int rows = a->vt ? a->L_pad : a->T;
    dim3 grid((rows + QK_TOK - 1) / QK_TOK, a->H), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == SVDQ_BF16)
        hipLaunchKernelGGL((qk_norm_rope_kernel<SVDQ_BF16>), grid, block, 0, st, (uint16_t *)a->qkv, (const uint16_t *)a->norm_q, (const uint16_t *)a->norm_k,
                           a->freqs, (uint16_t *)a->vt, a->rstd, a->ld, a->ldvt, a->T, a->L_pad, a->H, a->eps);
    else
        hipLaunchKernelGGL((qk_norm_rope_kernel<SVDQ_FP16>), grid, block, 0, st, (uint16_t *)a->qkv, (const uint16_t *)a->norm_q, (const uint16_t *)a->norm_k,
                           a->freqs, (uint16_t *)a->vt, a->rstd, a->ld, a->ldvt, a->T, a->L_pad, a->H, a->eps);
    return hip_check(hipGetLastError(), "svdq_qk_norm_rope launch");
}
