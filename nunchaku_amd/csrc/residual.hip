// svdq_residual_gate_stats: the element-wise glue between the operators of a FLUX block, with the statistics of the
// NEXT LayerNorm produced in the same pass (extension; reference blocks: transformer_flux_v2.py:118-342 use
// torch ops: hidden + gate * attn_out, LayerNorm, (1 + scale) * x + shift).
//
//   t = b ? round16(a + b) : a;   y = a ? round16(res + round16(gate * t)) : res;   out = y;   stats = (mean, rstd) of y
// (the rounding points of the reference's 16-bit torch ops: `attn + mlp`, `gate * x`, `residual + x`,
//  transformer_flux_v2.py:230-251,332-335)
//
// HBM-bound: one pass over the row (3 reads + 1 write of 2 bytes per element); one wave per row keeps the whole
// row in registers (C <= 16384), so mean and variance are the exact two-pass formulas on the stored 16-bit values
// and the LayerNorm itself disappears into the quantiser (svdq_quantize_args.ln_stats).
#include "row_pass.h"

namespace svdq {

template <int DT, int NV /* 16-byte pieces per lane */>
__global__ __launch_bounds__(256) void residual_kernel(const uint16_t *__restrict__ res, const uint16_t *__restrict__ a,
                                                        const uint16_t *__restrict__ b, const uint16_t *__restrict__ gate,
                                                        uint16_t *__restrict__ out, float *__restrict__ stats, int M, int C, int ld,
                                                        float eps, v4i *__restrict__ zero_ptr, long long zero_vec,
                                                        const uint16_t *__restrict__ res2, const uint16_t *__restrict__ a2,
                                                        const uint16_t *__restrict__ b2, const uint16_t *__restrict__ gate2,
                                                        uint16_t *__restrict__ out2, float *__restrict__ stats2, int M2, int clamp) {
    using T = typename Half<DT>::T;
    // side job: clear the scratch buffer, 16 bytes per thread, grid-strided (before any early return)
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < zero_vec; i += (long long)gridDim.x * 256) zero_ptr[i] = v4i{0, 0, 0, 0};
    const int lane = threadIdx.x & 63;
    int row = wave_row();
    if (row >= M) { // grouped launch: the second problem's rows
        if (!second_problem_row(row, M, res2, M2)) return;
        res = res2; a = a2; b = b2; gate = gate2; out = out2; stats = stats2;
        clamp >>= 1;
    }
    // fp16 only: y = clip(y, +-65504) like the reference's blocks (transformer_flux_v2.py:254-255, 339-340): an overflowed
    // sum is stored as the largest finite value and the statistics see that value, not inf
    const bool clip = DT == SVDQ_FP16 && (clamp & 1);
    const size_t base = (size_t)row * ld;
    float y[NV][8];
    float sum = 0.f;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const int c = (v * 64 + lane) * 8; // piece v of this lane (row_pass.h)
        if (c >= C) { // ragged tail of the last pass
#pragma unroll
            for (int e = 0; e < 8; e++) y[v][e] = 0.f;
            continue;
        }
        const u16x8 rv = ld8(res + base + c);
        if (a) {
            const u16x8 av = ld8(a + base + c);
            u16x8 bv, gv;
            if (b) bv = ld8(b + base + c);
            if (gate) gv = ld8(gate + c);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float t = h2f(hfrom<T>(av[e]));
                if (b) t = round16<T>(t + h2f(hfrom<T>(bv[e])));
                if (gate) t = round16<T>(h2f(hfrom<T>(gv[e])) * t);
                y[v][e] = round16<T>(h2f(hfrom<T>(rv[e])) + t);
                if (clip) y[v][e] = fminf(fmaxf(y[v][e], -65504.f), 65504.f);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) y[v][e] = h2f(hfrom<T>(rv[e]));
        }
        if (out && a) {
            u16x8 ov;
#pragma unroll
            for (int e = 0; e < 8; e++) ov[e] = hbits(f2h<T>(y[v][e]));
            st8(out + base + c, ov);
        }
#pragma unroll
        for (int e = 0; e < 8; e++) sum += y[v][e];
    }
    if (!stats) return;
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
    if (lane == 0) {
        stats[2 * (size_t)row] = mean;
        stats[2 * (size_t)row + 1] = 1.0f / sqrtf(sq / (float)C + eps);
    }
}

static bool launch_residual(const svdq_residual_args *p, hipStream_t st) {
    dim3 grid((p->M + (p->res2 ? p->M2 : 0) + 3) / 4), block(256);
    return for_row_class(p->dtype, p->C, [&](auto dt, auto nv) {
        hipLaunchKernelGGL((residual_kernel<decltype(dt)::value, decltype(nv)::value>), grid, block, 0, st, (const uint16_t *)p->res,
                           (const uint16_t *)p->a, (const uint16_t *)p->b, (const uint16_t *)p->gate, (uint16_t *)p->out, p->stats, p->M, p->C,
                           p->ld, p->eps, (v4i *)p->zero_ptr, (long long)(p->zero_ptr ? p->zero_bytes / 16 : 0), (const uint16_t *)p->res2,
                           (const uint16_t *)p->a2, (const uint16_t *)p->b2, (const uint16_t *)p->gate2, (uint16_t *)p->out2, p->stats2, p->M2,
                           p->clamp_fp16);
    });
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_residual_gate_stats(const svdq_residual_args *a, void *stream) {
    const char *op = "svdq_residual_gate_stats";
    if (!a) { set_error("%s: args is NULL", op); return SVDQ_E_INVALID; }
    if (!a->res || (!a->out && !a->stats)) { set_error("%s: res and one of out / stats are required", op); return SVDQ_E_INVALID; }
    if ((a->b || a->gate || a->out) && !a->a) { set_error("%s: b, gate and out need a", op); return SVDQ_E_INVALID; }
    if (int rc = check_row_args(op, a->M, a->C, a->ld, a->dtype, {a->res, a->a, a->b, a->gate, a->out}, {a->stats})) return rc;
    if (a->zero_ptr && (a->zero_bytes < 0 || a->zero_bytes % 16 || ((uintptr_t)a->zero_ptr & 15))) {
        set_error("%s: zero_ptr must be 16-byte aligned and zero_bytes a non-negative multiple of 16", op);
        return SVDQ_E_INVALID;
    }
    if (a->res2)
        if (int rc = check_second_problem(op, a->M2, a->res2, {{a->a, a->a2}, {a->b, a->b2}, {a->gate, a->gate2}, {a->out, a->out2}},
                                          {{a->stats, a->stats2}}))
            return rc;
    if (!launch_residual(a, (hipStream_t)stream)) return row_class_unsupported(op, a->C);
    return hip_check(hipGetLastError(), "svdq_residual_gate_stats launch");
}
