// svdq_sandwich_norm: the element-wise glue around the two sub-layers of a Z-Image block (diffusers ZImageTransformerBlock: four full-width
// RMSNorms in a sandwich around attention and feed-forward, two per-sample modulations, two tanh-gated residuals -- some twenty 16-bit torch
// passes per block).  One pass over a row closes a sub-layer and opens the next:
//
//   rms(h, w)[c] = round16(round16(h[c] * rstd(h)) * w[c]),   rstd(h) = 1 / sqrt(mean_c(h[c]^2) + eps)
//   y       = a ? round16(res + (gate ? round16(gate[b] * rms(a, w_post)) : rms(a, w_post))) : res        -> out
//   out_mod = scale ? round16(rms(y, w_pre) * scale[b]) : rms(y, w_pre)                                     -> out_mod
//   stats[row] = (rstd(a) or 0, rstd(y))
//
// Every operation between two roundings is one plain fp32 multiply or add (the library is built with -ffp-contract=off); for fp16 the fp32
// result is kept from being folded with the conversion behind it (op32), so both dtypes round twice -- to fp32, then to 16 bits -- exactly
// as the 16-bit torch operations they restate.  No fp16 clipping: diffusers has none here.
//
// HBM-bound: up to 2 reads + 2 writes of 2 bytes per element; the weights and the per-sample vectors stay in cache.  One wave per row keeps
// the row in registers AS 16-BIT PIECES (four registers per piece, 128 for the widest class): first a, then y in the same registers.  Row r
// belongs to sample r / T, so the four rows of a workgroup may read two samples' vectors.  The sums of squares run in one fixed order: a lane
// adds its elements in index order, the 6-level butterfly folds the wave.  No LDS, no atomics.
#include <cmath>

#include "row_pass.h"

namespace svdq {

// the fp32 result of one operation, opaque to the optimiser for fp16: (T)(x * y) must stay v_mul_f32 + v_cvt_f16_f32 (two roundings), not
// become one v_fma_mix that rounds once
template <typename T> __device__ __forceinline__ float op32(float v) {
    if constexpr (__is_same(T, _Float16)) asm("" : "+v"(v));
    return v;
}
template <typename T> __device__ __forceinline__ float mul16(float x, float y) { return round16<T>(op32<T>(x * y)); }

// sum of the squares of the row held in yv (zero pieces beyond C), in the fixed order, folded over the wave; -> rstd
template <typename T16, int NV> __device__ __forceinline__ float row_rstd(const u16x8 (&yv)[NV], int C, float eps) {
    float sq = 0.f;
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const float x = h2f(hfrom<T16>(yv[v][e]));
            sq = sq + x * x;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    return 1.0f / sqrtf(sq / (float)C + eps);
}

template <int DT, int NV /* 16-byte pieces per lane */>
__global__ __launch_bounds__(256) void sandwich_norm_kernel(const uint16_t *res, const uint16_t *__restrict__ a, const uint16_t *__restrict__ w_post,
                                                             const uint16_t *__restrict__ gate, const uint16_t *__restrict__ w_pre,
                                                             const uint16_t *__restrict__ scale, uint16_t *out, uint16_t *__restrict__ out_mod,
                                                             float *__restrict__ stats, long long gate_bs, long long scale_bs, int ld_res, int ld_a,
                                                             int ld_out, int ld_mod, int M, int T, int C, float eps) {
    using T16 = typename Half<DT>::T;
    const int lane = threadIdx.x & 63;
    const int row = wave_row();
    if (row >= M) return; // (wave-uniform)
    const size_t b = (size_t)(row / T); // this row's sample
    const size_t o_res = (size_t)row * ld_res, o_a = (size_t)row * ld_a, o_out = (size_t)row * ld_out, o_mod = (size_t)row * ld_mod;
    const u16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    u16x8 yv[NV];
    float rstd_a = 0.f;
    if (a) {
#pragma unroll
        for (int v = 0; v < NV; v++) {
            const int c = (v * 64 + lane) * 8; // piece v of this lane (row_pass.h)
            yv[v] = c < C ? ld8(a + o_a + c) : zero;
        }
        rstd_a = row_rstd<T16, NV>(yv, C, eps);
        const uint16_t *g = gate ? gate + b * (size_t)gate_bs : nullptr;
#pragma unroll
        for (int v = 0; v < NV; v++) {
            const int c = (v * 64 + lane) * 8;
            if (c >= C) continue;
            const u16x8 rv = ld8(res + o_res + c), wv = ld8(w_post + c);
            u16x8 gv = zero;
            if (g) gv = ld8(g + c);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float n = mul16<T16>(mul16<T16>(h2f(hfrom<T16>(yv[v][e])), rstd_a), h2f(hfrom<T16>(wv[e])));
                if (g) n = mul16<T16>(h2f(hfrom<T16>(gv[e])), n);
                yv[v][e] = hbits(f2h<T16>(op32<T16>(h2f(hfrom<T16>(rv[e])) + n)));
            }
            if (out) st8(out + o_out + c, yv[v]);
        }
    } else {
#pragma unroll
        for (int v = 0; v < NV; v++) {
            const int c = (v * 64 + lane) * 8;
            yv[v] = c < C ? ld8(res + o_res + c) : zero;
            if (out && c < C) st8(out + o_out + c, yv[v]);
        }
    }
    if (!stats && !out_mod) return;
    const float rstd_y = row_rstd<T16, NV>(yv, C, eps);
    if (stats && lane == 0) {
        stats[2 * (size_t)row] = rstd_a;
        stats[2 * (size_t)row + 1] = rstd_y;
    }
    if (!out_mod) return;
    const uint16_t *s = scale ? scale + b * (size_t)scale_bs : nullptr;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const int c = (v * 64 + lane) * 8;
        if (c >= C) continue;
        const u16x8 wv = ld8(w_pre + c);
        u16x8 sv = zero, mv;
        if (s) sv = ld8(s + c);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            float m = mul16<T16>(mul16<T16>(h2f(hfrom<T16>(yv[v][e])), rstd_y), h2f(hfrom<T16>(wv[e])));
            if (s) m = mul16<T16>(m, h2f(hfrom<T16>(sv[e])));
            mv[e] = hbits(f2h<T16>(m));
        }
        st8(out_mod + o_mod + c, mv);
    }
}

static bool launch_sandwich_norm(const svdq_sandwich_norm_args *p, hipStream_t st) {
    dim3 grid((p->M + 3) / 4), block(256);
    return for_row_class(p->dtype, p->C, [&](auto dt, auto nv) {
        hipLaunchKernelGGL((sandwich_norm_kernel<decltype(dt)::value, decltype(nv)::value>), grid, block, 0, st, (const uint16_t *)p->res,
                           (const uint16_t *)p->a, (const uint16_t *)p->w_post, (const uint16_t *)p->gate, (const uint16_t *)p->w_pre,
                           (const uint16_t *)p->scale, (uint16_t *)p->out, (uint16_t *)p->out_mod, p->stats, (long long)p->gate_bs,
                           (long long)p->scale_bs, p->ld_res, p->ld_a, p->ld_out, p->ld_mod, p->M, p->T, p->C, p->eps);
    });
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_sandwich_norm(const svdq_sandwich_norm_args *a, void *stream) {
    const char *op = "svdq_sandwich_norm";
    if (!a) { set_error("%s: args is NULL", op); return SVDQ_E_INVALID; }
    if (!a->res || (!a->out && !a->out_mod && !a->stats)) { set_error("%s: res and one of out / out_mod / stats are required", op); return SVDQ_E_INVALID; }
    if (a->gate && !a->a) { set_error("%s: gate needs a", op); return SVDQ_E_INVALID; }
    if (a->a && !a->w_post) { set_error("%s: a needs w_post", op); return SVDQ_E_INVALID; }
    if (a->out_mod && !a->w_pre) { set_error("%s: out_mod needs w_pre", op); return SVDQ_E_INVALID; }
    // every tensor of rows has its own stride: the shared checks, once per stride
    if (int rc = check_row_args(op, a->M, a->C, a->ld_res, a->dtype, {a->res, a->a, a->w_post, a->gate, a->w_pre, a->scale, a->out, a->out_mod}, {a->stats})) return rc;
    if (a->a) if (int rc = check_row_args(op, a->M, a->C, a->ld_a, a->dtype, {}, {})) return rc;
    if (a->out) if (int rc = check_row_args(op, a->M, a->C, a->ld_out, a->dtype, {}, {})) return rc;
    if (a->out_mod) if (int rc = check_row_args(op, a->M, a->C, a->ld_mod, a->dtype, {}, {})) return rc;
    if (a->T < 1 || a->M % a->T) { set_error("%s: M=%d rows are not whole samples of T=%d rows", op, a->M, a->T); return SVDQ_E_INVALID; }
    const bool uses_scale = a->scale && a->out_mod;
    if ((a->gate && (a->gate_bs < a->C || a->gate_bs % 8)) || (uses_scale && (a->scale_bs < a->C || a->scale_bs % 8))) {
        set_error("%s: gate_bs=%lld and scale_bs=%lld must be at least C=%d and multiples of 8", op, (long long)a->gate_bs, (long long)a->scale_bs, a->C);
        return SVDQ_E_INVALID;
    }
    if (!(a->eps >= 0.f) || !std::isfinite(a->eps)) { set_error("%s: eps must be finite and not negative", op); return SVDQ_E_INVALID; }
    if (!launch_sandwich_norm(a, (hipStream_t)stream)) return row_class_unsupported(op, a->C);
    return hip_check(hipGetLastError(), "svdq_sandwich_norm launch");
}
