// svdq_sana_glue: the element-wise glue between the three layers of a SANA block (reference: SanaLinearTransformerBlock::forward,
// src/SanaModel.cpp:234-322 -- a copy of timestep, one add of scale_shift_table, two LayerNorms and five mul_add_batch launches per block).
// One pass over a row does the gated residual, the LayerNorm of the result, the NEXT layer's per-sample modulation and the padding of both
// outputs to the width of the 4-bit GEMM's operand (SANA-1.6B: 2240 channels in 2304-wide rows):
//
//   mod(tab, i)[b, c] = clip(round16(timestep[b, i, c] + tab[i, c]))
//   t = res | clip(round16(a + res)) | clip(round16(round16(a * mod(gate_table, gate_row)[b]) + res));   out[r, :C] = t, out[r, C:C_pad] = 0
//   (mean, rstd) = two-pass fp32 statistics of t (residual_kernel's);   n = round16((t - mean) * rstd)
//   out_mod[r, :C] = clip(round16(round16(n * round16(mod(mod_table, scale_row)[b] + 1)) + mod(mod_table, shift_row)[b])), tail 0
//
// with the rounding points of the reference's separate operations (include/svdq_amd.h says which; nvcc may contract the reference's
// multiply-add, this project fixes the reading above).  clip: +-65504 for fp16, nothing for bf16 (misc_kernels_impl.cuh:60-63).
//
// HBM-bound: 2 reads + up to 2 writes of 2 bytes per element; the modulation vectors (6 x C per sample and table) stay in cache.  One wave
// per row keeps the row in registers (row_pass.h); row r belongs to sample r / T, so the four rows of a workgroup may read two samples'
// vectors.  The width class is that of C_pad: the lanes at C <= c < C_pad store zeros, the lanes at c >= C_pad do nothing.  No LDS, no atomics.
#include <cmath>

#include "row_pass.h"

namespace svdq {

template <int DT> __device__ __forceinline__ float clip16(float v) {
    return DT == SVDQ_FP16 ? fminf(fmaxf(v, -65504.f), 65504.f) : v;
}
// mod(tab, i)[b] for the eight columns of one piece: tv = timestep[b, i, c ..], bv = tab[i, c ..]
template <int DT> __device__ __forceinline__ float mod16(unsigned short tv, unsigned short bv) {
    using T = typename Half<DT>::T;
    return clip16<DT>(round16<T>(h2f(hfrom<T>(tv)) + h2f(hfrom<T>(bv))));
}

template <int DT, int NV /* 16-byte pieces per lane */>
__global__ __launch_bounds__(256) void sana_glue_kernel(const uint16_t *res, const uint16_t *__restrict__ a, const uint16_t *__restrict__ timestep,
                                                         const uint16_t *__restrict__ gate_table, const uint16_t *__restrict__ mod_table,
                                                         uint16_t *out, uint16_t *__restrict__ out_mod, float *__restrict__ stats, long long ts_bs,
                                                         int ld_res, int ld_a, int ld_out, int ld_mod, int M, int T, int C, int C_pad, int gate_row,
                                                         int scale_row, int shift_row, float eps) {
    using T16 = typename Half<DT>::T;
    const int lane = threadIdx.x & 63;
    const int row = wave_row();
    if (row >= M) return; // (wave-uniform)
    const uint16_t *ts = timestep ? timestep + (size_t)(row / T) * (size_t)ts_bs : nullptr; // this row's sample
    const size_t o_res = (size_t)row * ld_res, o_a = (size_t)row * ld_a, o_out = (size_t)row * ld_out, o_mod = (size_t)row * ld_mod;
    const bool gated = a && gate_row >= 0;
    const u16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    float y[NV][8];
    float sum = 0.f;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const int c = (v * 64 + lane) * 8; // piece v of this lane (row_pass.h)
        if (c >= C) {                      // the zero tail up to C_pad, nothing beyond it
#pragma unroll
            for (int e = 0; e < 8; e++) y[v][e] = 0.f;
            if (out && c < C_pad) st8(out + o_out + c, zero);
            continue;
        }
        const u16x8 rv = ld8(res + o_res + c);
        if (a) {
            const u16x8 av = ld8(a + o_a + c);
            u16x8 gt, gb;
            if (gated) { gt = ld8(ts + (size_t)gate_row * C + c); gb = ld8(gate_table + (size_t)gate_row * C + c); }
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float t = h2f(hfrom<T16>(av[e]));
                if (gated) t = round16<T16>(t * mod16<DT>(gt[e], gb[e]));
                y[v][e] = clip16<DT>(round16<T16>(t + h2f(hfrom<T16>(rv[e]))));
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) y[v][e] = h2f(hfrom<T16>(rv[e]));
        }
        if (out) {
            u16x8 ov;
#pragma unroll
            for (int e = 0; e < 8; e++) ov[e] = hbits(f2h<T16>(y[v][e]));
            st8(out + o_out + c, ov);
        }
#pragma unroll
        for (int e = 0; e < 8; e++) sum += y[v][e];
    }
    if (!stats && !out_mod) return;
    // the statistics, operation for operation as residual_kernel forms them
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float mean = sum / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const float d = (v * 64 + lane) * 8 < C ? y[v][e] - mean : 0.f;
            sq = __builtin_fmaf(d, d, sq);
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    const float rstd = 1.0f / sqrtf(sq / (float)C + eps);
    if (stats && lane == 0) {
        stats[2 * (size_t)row] = mean;
        stats[2 * (size_t)row + 1] = rstd;
    }
    if (!out_mod) return;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const int c = (v * 64 + lane) * 8;
        if (c >= C) {
            if (c < C_pad) st8(out_mod + o_mod + c, zero);
            continue;
        }
        const u16x8 st = ld8(ts + (size_t)scale_row * C + c), sb = ld8(mod_table + (size_t)scale_row * C + c);
        const u16x8 ht = ld8(ts + (size_t)shift_row * C + c), hb = ld8(mod_table + (size_t)shift_row * C + c);
        u16x8 mv;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const float n = round16<T16>((y[v][e] - mean) * rstd);
            const float s = round16<T16>(mod16<DT>(st[e], sb[e]) + 1.0f);
            const float m = round16<T16>(round16<T16>(n * s) + mod16<DT>(ht[e], hb[e]));
            mv[e] = hbits(f2h<T16>(clip16<DT>(m)));
        }
        st8(out_mod + o_mod + c, mv);
    }
}

static bool launch_sana_glue(const svdq_sana_glue_args *p, hipStream_t st) {
    const int M = p->B * p->T;
    dim3 grid((M + 3) / 4), block(256);
    return for_row_class(p->dtype, p->C_pad, [&](auto dt, auto nv) {
        hipLaunchKernelGGL((sana_glue_kernel<decltype(dt)::value, decltype(nv)::value>), grid, block, 0, st, (const uint16_t *)p->res,
                           (const uint16_t *)p->a, (const uint16_t *)p->timestep, (const uint16_t *)p->gate_table,
                           (const uint16_t *)p->mod_table, (uint16_t *)p->out, (uint16_t *)p->out_mod, p->stats, (long long)p->timestep_bs,
                           p->ld_res, p->ld_a, p->ld_out, p->ld_mod, M, p->T, p->C, p->C_pad, p->a ? p->gate_row : -1, p->scale_row,
                           p->shift_row, p->eps);
    });
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_sana_glue(const svdq_sana_glue_args *a, void *stream) {
    const char *op = "svdq_sana_glue";
    if (!a) { set_error("%s: args is NULL", op); return SVDQ_E_INVALID; }
    if (!a->res || (!a->out && !a->out_mod && !a->stats)) { set_error("%s: res and one of out / out_mod / stats are required", op); return SVDQ_E_INVALID; }
    const bool gated = a->gate_row >= 0;
    if (gated && !a->a) { set_error("%s: gate_row=%d needs a", op, a->gate_row); return SVDQ_E_INVALID; }
    if (a->gate_row > 5 || (a->out_mod && (a->scale_row < 0 || a->scale_row > 5 || a->shift_row < 0 || a->shift_row > 5))) {
        set_error("%s: gate_row=%d, scale_row=%d, shift_row=%d: table rows are 0..5 (gate_row < 0: no gate)", op, a->gate_row, a->scale_row, a->shift_row);
        return SVDQ_E_INVALID;
    }
    if (a->out_mod && (!a->timestep || !a->mod_table)) { set_error("%s: out_mod needs timestep and mod_table", op); return SVDQ_E_INVALID; }
    if (gated && (!a->timestep || !a->gate_table)) { set_error("%s: a gate needs timestep and gate_table", op); return SVDQ_E_INVALID; }
    if (a->B < 1 || a->T < 1 || a->C < 1 || (long long)a->B * a->T > 0x7fffffffLL) {
        set_error("%s: need B=%d, T=%d, C=%d >= 1 and B * T < 2^31", op, a->B, a->T, a->C);
        return SVDQ_E_INVALID;
    }
    if (a->C > a->C_pad || a->C % 8 || a->C_pad % 8) {
        set_error("%s: need C=%d <= C_pad=%d, both multiples of 8", op, a->C, a->C_pad);
        return SVDQ_E_INVALID;
    }
    const bool uses_ts = gated || a->out_mod;
    if (a->ld_res < a->C || (a->a && a->ld_a < a->C) || (a->out && a->ld_out < a->C_pad) || (a->out_mod && a->ld_mod < a->C_pad) ||
        (uses_ts && a->timestep_bs < 6LL * a->C)) {
        set_error("%s: a stride is smaller than its row: ld_res=%d, ld_a=%d (C=%d), ld_out=%d, ld_mod=%d (C_pad=%d), timestep_bs=%lld (6 * C)", op,
                  a->ld_res, a->ld_a, a->C, a->ld_out, a->ld_mod, a->C_pad, (long long)a->timestep_bs);
        return SVDQ_E_INVALID;
    }
    if (a->ld_res % 8 || (a->a && a->ld_a % 8) || (a->out && a->ld_out % 8) || (a->out_mod && a->ld_mod % 8) || (uses_ts && a->timestep_bs % 8)) {
        set_error("%s: every stride must be a multiple of 8 elements", op);
        return SVDQ_E_INVALID;
    }
    if (!aligned_to(16, {a->res, a->a, a->timestep, a->gate_table, a->mod_table, a->out, a->out_mod}) || !aligned_to(8, {a->stats})) {
        set_error("%s: 16-bit tensors must be 16-byte aligned, stats 8-byte aligned", op);
        return SVDQ_E_INVALID;
    }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("%s: unknown dtype %d", op, a->dtype); return SVDQ_E_INVALID; }
    if (!(a->eps >= 0.f) || !std::isfinite(a->eps)) { set_error("%s: eps must be finite and not negative", op); return SVDQ_E_INVALID; }
    if (!launch_sana_glue(a, (hipStream_t)stream)) return row_class_unsupported(op, a->C_pad);
    return hip_check(hipGetLastError(), "svdq_sana_glue launch");
}
