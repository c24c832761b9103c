// svdq_modulated_diff: the decision pass of TeaCache (reference: nunchaku/caching/teacache.py:187,199-200 -- block 0's AdaLayerNormZero
// output and `(m - prev).abs().mean() / prev.abs().mean()`: a LayerNorm, a multiply, an add and the six launches of the distance there, one
// pass here).  On the fused path the modulated input of a block exists only inside the quantiser's front end; this kernel restates that
// front end with its rounding points (quantize.hip; oracle ln_mod_ref) from the row statistics the engine already has:
//
//   m = round16(round16(round16((x - mean) * rstd) * mod_scale) + mod_shift);   out_mod = m (if given);
//   sum_diff += |round16(prev - m)|;   sum_prev += |prev|        (if prev is given)
//
// HBM-bound: 2 reads + 1 write of 2 bytes per element (the two [C] vectors stay in cache).  One wave per row in 16-byte pieces
// (row_pass.h); nothing of the row is kept (the statistics are an input).  prev and out_mod may be the same buffer: a lane reads its piece
// of prev before it writes that piece of out_mod, and no other lane touches it.  The sums take the decision tail of row_pass.h, the code
// svdq_residual_diff runs: add_distance in index order, store_row_pair, launch_diff_reduce behind it on the same stream -- no floating-point
// atomics, at most  8 * ceil(C / 512) + 6 + ceil(M / 256) + 8  additions per term.
#include "row_pass.h"

namespace svdq {

template <int DT, int NV /* 16-byte pieces per lane */>
__global__ __launch_bounds__(256) void modulated_diff_kernel(const uint16_t *x, const float *__restrict__ stats, const uint16_t *__restrict__ mod_scale,
                                                              const uint16_t *__restrict__ mod_shift, const uint16_t *prev, uint16_t *out, int M,
                                                              int C, int ld, float *__restrict__ partials) {
    using T = typename Half<DT>::T;
    const int lane = threadIdx.x & 63;
    const int row = wave_row();
    if (row >= M) return; // (wave-uniform)
    const size_t off = (size_t)row * ld;
    const float2 st = *reinterpret_cast<const float2 *>(stats + 2 * (size_t)row);
    const float mean = st.x, rstd = st.y;
    float sd = 0.f, sp = 0.f;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const int c = (v * 64 + lane) * 8; // piece v of this lane (row_pass.h)
        if (c >= C) continue;              // ragged tail of the last pass
        const u16x8 xv = ld8(x + off + c), sv = ld8(mod_scale + c), hv = ld8(mod_shift + c);
        u16x8 mv;
#pragma unroll
        for (int e = 0; e < 8; e++) { // the quantiser's front end, operation for operation
            const float ln = round16<T>((h2f(hfrom<T>(xv[e])) - mean) * rstd);
            const float y = round16<T>(ln * h2f(hfrom<T>(sv[e]))) + h2f(hfrom<T>(hv[e]));
            mv[e] = hbits(f2h<T>(y));
        }
        if (prev) add_distance<T>(ld8(prev + off + c), mv, sd, sp);
        if (out) st8(out + off + c, mv);
    }
    if (prev) store_row_pair(partials, row, lane, sd, sp);
}

static bool launch_modulated_diff(const svdq_modulated_diff_args *p, hipStream_t st) {
    dim3 grid((p->M + 3) / 4), block(256);
    const bool ok = for_row_class(p->dtype, p->C, [&](auto dt, auto nv) {
        hipLaunchKernelGGL((modulated_diff_kernel<decltype(dt)::value, decltype(nv)::value>), grid, block, 0, st, (const uint16_t *)p->x,
                           p->stats, (const uint16_t *)p->mod_scale, (const uint16_t *)p->mod_shift, (const uint16_t *)p->prev,
                           (uint16_t *)p->out_mod, p->M, p->C, p->ld, p->partials);
    });
    if (ok && p->prev) launch_diff_reduce(p->dtype, p->partials, p->M, p->C, p->result, st);
    return ok;
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_modulated_diff(const svdq_modulated_diff_args *a, void *stream) {
    const char *op = "svdq_modulated_diff";
    if (!a) { set_error("%s: args is NULL", op); return SVDQ_E_INVALID; }
    if (!a->x || !a->stats || !a->mod_scale || !a->mod_shift) { set_error("%s: x, stats, mod_scale and mod_shift are required", op); return SVDQ_E_INVALID; }
    if (!a->out_mod && !a->prev) { set_error("%s: one of out_mod / prev is required", op); return SVDQ_E_INVALID; }
    if (a->prev && (!a->result || !a->partials)) {
        set_error("%s: prev needs a result record and the partials buffer ([M, 2] fp32)", op);
        return SVDQ_E_INVALID;
    }
    if (int rc = check_row_args(op, a->M, a->C, a->ld, a->dtype, {a->x, a->mod_scale, a->mod_shift, a->prev, a->out_mod},
                                {a->stats, a->partials, a->result}))
        return rc;
    if (!launch_modulated_diff(a, (hipStream_t)stream)) return row_class_unsupported(op, a->C);
    return hip_check(hipGetLastError(), "svdq_modulated_diff launch");
}
