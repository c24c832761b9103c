// svdq_modulated_diff: the decision pass of TeaCache (reference: nunchaku/caching/teacache.py:187,199-200 -- block 0's AdaLayerNormZero
// output and `(m - prev).abs().mean() / prev.abs().mean()`: a LayerNorm, a multiply, an add and the six launches of the distance there, one
// pass here).  On the fused path the modulated input of a block exists only inside the quantiser's front end; this kernel restates that
// front end with its rounding points (quantize.hip; oracle ln_mod_ref) from the row statistics the engine already has:
//
//   m = round16(round16(round16((x - mean) * rstd) * mod_scale) + mod_shift);   out_mod = m (if given);
//   sum_diff += |round16(prev - m)|;   sum_prev += |prev|        (if prev is given)
//
// HBM-bound: 2 reads + 1 write of 2 bytes per element (the two [C] vectors stay in cache).  One wave per row, 16-byte pieces, as
// residual_diff_kernel; nothing of the row is kept (the statistics are an input).  prev and out_mod may be the same buffer: a lane reads
// its piece of prev before it writes that piece of out_mod, and no other lane touches it.  The sums take residual_diff's route: a lane
// adds its elements in index order, fold_wave_pair, the row's pair to `partials`, launch_diff_reduce behind it on the same stream --
// no floating-point atomics, at most  8 * ceil(C / 512) + 6 + ceil(M / 256) + 8  additions per term.
#include "svdq_common.h"

namespace svdq {

template <int DT, int NV /* 16-byte pieces per lane */>
__global__ __launch_bounds__(256) void modulated_diff_kernel(const uint16_t *x, const float *__restrict__ stats, const uint16_t *__restrict__ mod_scale,
                                                              const uint16_t *__restrict__ mod_shift, const uint16_t *prev, uint16_t *out, int M,
                                                              int C, int ld, float *__restrict__ partials) {
    using T = typename Half<DT>::T;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return; // (wave-uniform)
    const size_t off = (size_t)row * ld;
    const float2 st = *reinterpret_cast<const float2 *>(stats + 2 * (size_t)row);
    const float mean = st.x, rstd = st.y;
    float sd = 0.f, sp = 0.f;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const int c = (v * 64 + lane) * 8; // a wave instruction covers 1 KiB of the row
        if (c >= C) continue;              // ragged tail of the last pass (C is a multiple of 8, not necessarily of 512)
        const u16x8 xv = *reinterpret_cast<const u16x8 *>(x + off + c);
        const u16x8 sv = *reinterpret_cast<const u16x8 *>(mod_scale + c);
        const u16x8 hv = *reinterpret_cast<const u16x8 *>(mod_shift + c);
        u16x8 mv;
#pragma unroll
        for (int e = 0; e < 8; e++) { // the quantiser's front end, operation for operation
            const float ln = round16<T>((h2f(hfrom<T>(xv[e])) - mean) * rstd);
            const float y = round16<T>(ln * h2f(hfrom<T>(sv[e]))) + h2f(hfrom<T>(hv[e]));
            mv[e] = hbits(f2h<T>(y));
        }
        if (prev) {
            const u16x8 pv = *reinterpret_cast<const u16x8 *>(prev + off + c);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float p = h2f(hfrom<T>(pv[e]));
                sd += fabsf(round16<T>(p - h2f(hfrom<T>(mv[e]))));
                sp += fabsf(p);
            }
        }
        if (out) *reinterpret_cast<u16x8 *>(out + off + c) = mv;
    }
    if (!prev) return;
    fold_wave_pair(sd, sp);
    if (lane == 0) {
        partials[2 * (size_t)row] = sd;
        partials[2 * (size_t)row + 1] = sp;
    }
}

template <int DT> static int launch_modulated_diff(const svdq_modulated_diff_args *p, hipStream_t st) {
    dim3 grid((p->M + 3) / 4), block(256);
#define SVDQ_MDIFF_CASE(NV)                                                                                                          \
    case NV:                                                                                                                         \
        hipLaunchKernelGGL((modulated_diff_kernel<DT, NV>), grid, block, 0, st, (const uint16_t *)p->x, p->stats,                     \
                           (const uint16_t *)p->mod_scale, (const uint16_t *)p->mod_shift, (const uint16_t *)p->prev,                 \
                           (uint16_t *)p->out_mod, p->M, p->C, p->ld, p->partials);                                                   \
        break;
    switch ((p->C + 511) / 512) {
        SVDQ_MDIFF_CASE(1) SVDQ_MDIFF_CASE(2) SVDQ_MDIFF_CASE(3) SVDQ_MDIFF_CASE(4) SVDQ_MDIFF_CASE(5) SVDQ_MDIFF_CASE(6) SVDQ_MDIFF_CASE(7) SVDQ_MDIFF_CASE(8)
        SVDQ_MDIFF_CASE(12) SVDQ_MDIFF_CASE(16) SVDQ_MDIFF_CASE(24) SVDQ_MDIFF_CASE(32)
    default: return -1;
    }
#undef SVDQ_MDIFF_CASE
    if (p->prev) launch_diff_reduce(DT, p->partials, p->M, p->C, p->result, st);
    return 0;
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_modulated_diff(const svdq_modulated_diff_args *a, void *stream) {
    if (!a) { set_error("svdq_modulated_diff: args is NULL"); return SVDQ_E_INVALID; }
    if (!a->x || !a->stats || !a->mod_scale || !a->mod_shift) {
        set_error("svdq_modulated_diff: x, stats, mod_scale and mod_shift are required");
        return SVDQ_E_INVALID;
    }
    if (!a->out_mod && !a->prev) { set_error("svdq_modulated_diff: one of out_mod / prev is required"); return SVDQ_E_INVALID; }
    if (a->prev && (!a->result || !a->partials)) {
        set_error("svdq_modulated_diff: prev needs a result record and the partials buffer ([M, 2] fp32)");
        return SVDQ_E_INVALID;
    }
    if (a->M <= 0 || a->C <= 0 || a->C % 8 || a->ld < a->C || a->ld % 8) {
        set_error("svdq_modulated_diff: need M=%d > 0, C=%d a multiple of 8, ld=%d >= C and a multiple of 8", a->M, a->C, a->ld);
        return SVDQ_E_INVALID;
    }
    if (((uintptr_t)a->x | (uintptr_t)a->mod_scale | (uintptr_t)a->mod_shift | (uintptr_t)a->prev | (uintptr_t)a->out_mod) & 15 ||
        ((uintptr_t)a->stats & 7) || ((uintptr_t)a->partials & 7) || ((uintptr_t)a->result & 7)) {
        set_error("svdq_modulated_diff: tensors must be 16-byte aligned (stats, partials and result 8-byte)");
        return SVDQ_E_INVALID;
    }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("svdq_modulated_diff: unknown dtype %d", a->dtype); return SVDQ_E_INVALID; }
    hipStream_t st = (hipStream_t)stream;
    const int rc = a->dtype == SVDQ_BF16 ? launch_modulated_diff<SVDQ_BF16>(a, st) : launch_modulated_diff<SVDQ_FP16>(a, st);
    if (rc) { set_error("svdq_modulated_diff: C=%d: ceil(C/512) must be one of {1..8, 12, 16, 24, 32}", a->C); return SVDQ_E_UNSUPPORTED; }
    return hip_check(hipGetLastError(), "svdq_modulated_diff launch");
}
