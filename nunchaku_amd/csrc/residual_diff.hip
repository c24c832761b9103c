// svdq_residual_diff: the decision pass of First-Block Cache (reference: nunchaku/caching/utils_v2.py:133,176 `hidden - original`,
// fbcache.py:275-277 `(t1 - t2).abs().mean() / t1.abs().mean()` -- six torch launches over the image stream there, one pass here).
//
//   r = base ? round16(cur - base) : cur;   out_res = r (if given);
//   sum_diff += |round16(prev - r)|;   sum_prev += |prev|        (if prev is given)
//
// HBM-bound: 3 reads + 1 write of 2 bytes per element.  One wave per row in 16-byte pieces (row_pass.h); nothing of the row is kept.
// The two sums are bit-reproducible: no floating-point atomics.  The lane sums, the wave's fold and the row's pair in `partials` are the
// decision tail of row_pass.h; the one-workgroup kernel of this file behind it on the same stream adds the rows in a fixed order (thread t:
// rows t, t + 256, ... in sequence; an 8-level tree over the 256 threads) and derives the 16-bit means and their quotient.  A term therefore
// passes through at most  8 * ceil(C / 512) + 6 + ceil(rows / 256) + 8  additions.
#include "row_pass.h"

namespace svdq {

template <int DT, int NV /* 16-byte pieces per lane */>
__global__ __launch_bounds__(256) void residual_diff_kernel(const uint16_t *cur, const uint16_t *base, const uint16_t *prev, uint16_t *out,
                                                             int M, int C, int ld, const uint16_t *cur2, const uint16_t *base2,
                                                             const uint16_t *prev2, uint16_t *out2, int M2, float *__restrict__ partials) {
    using T = typename Half<DT>::T;
    const int lane = threadIdx.x & 63;
    const int grow = wave_row(); // row of the grouped launch = index of its pair in `partials`
    int row = grow;
    if (row >= M) { // grouped launch: the second problem's rows
        if (!second_problem_row(row, M, cur2, M2)) return;
        cur = cur2; base = base2; prev = prev2; out = out2;
    }
    const size_t off = (size_t)row * ld;
    float sd = 0.f, sp = 0.f;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const int c = (v * 64 + lane) * 8; // piece v of this lane (row_pass.h)
        if (c >= C) continue;              // ragged tail of the last pass
        u16x8 rv = ld8(cur + off + c);
        if (base) {
            const u16x8 bv = ld8(base + off + c);
#pragma unroll
            for (int e = 0; e < 8; e++) rv[e] = hbits(f2h<T>(h2f(hfrom<T>(rv[e])) - h2f(hfrom<T>(bv[e]))));
        }
        if (prev) add_distance<T>(ld8(prev + off + c), rv, sd, sp);
        if (out) st8(out + off + c, rv);
    }
    if (prev) store_row_pair(partials, grow, lane, sd, sp);
}

// rows in a fixed order: thread t adds rows t, t + 256, ... one after the other, then a tree over the threads
template <int DT>
__global__ __launch_bounds__(256) void residual_diff_reduce_kernel(const float *__restrict__ partials, int rows, float inv_n,
                                                                    svdq_residual_diff_result *__restrict__ result) {
    using T = typename Half<DT>::T;
    __shared__ float sh[2][4];
    float sd = 0.f, sp = 0.f;
    for (int r = threadIdx.x; r < rows; r += 256) {
        sd += partials[2 * (size_t)r];
        sp += partials[2 * (size_t)r + 1];
    }
    fold_wave_pair(sd, sp);
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = sd; sh[1][threadIdx.x >> 6] = sp; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sd = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
        sp = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
        // torch's 16-bit mean: fp32 sum times 1/N, one rounding; the quotient of the two 16-bit means, one rounding
        const float md = round16<T>(sd * inv_n), mp = round16<T>(sp * inv_n);
        result->sum_diff = sd;
        result->sum_prev = sp;
        result->mean_diff = md;
        result->mean_prev = mp;
        result->ratio = round16<T>(md / mp);
        result->rows = rows;
        result->reserved[0] = result->reserved[1] = 0;
    }
}

static bool launch_residual_diff(const svdq_residual_diff_args *p, hipStream_t st) {
    const int rows = p->M + (p->cur2 ? p->M2 : 0);
    dim3 grid((rows + 3) / 4), block(256);
    const bool ok = for_row_class(p->dtype, p->C, [&](auto dt, auto nv) {
        hipLaunchKernelGGL((residual_diff_kernel<decltype(dt)::value, decltype(nv)::value>), grid, block, 0, st, (const uint16_t *)p->cur,
                           (const uint16_t *)p->base, (const uint16_t *)p->prev, (uint16_t *)p->out_res, p->M, p->C, p->ld,
                           (const uint16_t *)p->cur2, (const uint16_t *)p->base2, (const uint16_t *)p->prev2, (uint16_t *)p->out_res2, p->M2,
                           p->partials);
    });
    if (ok && p->prev) launch_diff_reduce(p->dtype, p->partials, rows, p->C, p->result, st);
    return ok;
}

void launch_diff_reduce(int dtype, const float *partials, int rows, int C, svdq_residual_diff_result *result, hipStream_t st) {
    const float inv_n = 1.0f / ((float)rows * (float)C);
    if (dtype == SVDQ_BF16) hipLaunchKernelGGL((residual_diff_reduce_kernel<SVDQ_BF16>), dim3(1), dim3(256), 0, st, partials, rows, inv_n, result);
    else hipLaunchKernelGGL((residual_diff_reduce_kernel<SVDQ_FP16>), dim3(1), dim3(256), 0, st, partials, rows, inv_n, result);
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_residual_diff(const svdq_residual_diff_args *a, void *stream) {
    const char *op = "svdq_residual_diff";
    if (!a) { set_error("%s: args is NULL", op); return SVDQ_E_INVALID; }
    if (!a->cur) { set_error("%s: cur is NULL", op); return SVDQ_E_INVALID; }
    if (!a->out_res && !a->prev) { set_error("%s: one of out_res / prev is required", op); return SVDQ_E_INVALID; }
    if (a->out_res && !a->base) { set_error("%s: out_res needs base (without base the residual is cur itself)", op); return SVDQ_E_INVALID; }
    if (a->prev && (!a->result || !a->partials)) {
        set_error("%s: prev needs a result record and the partials buffer ([M + M2, 2] fp32)", op);
        return SVDQ_E_INVALID;
    }
    if (int rc = check_row_args(op, a->M, a->C, a->ld, a->dtype, {a->cur, a->base, a->prev, a->out_res}, {a->partials, a->result})) return rc;
    if (a->cur2)
        if (int rc = check_second_problem(op, a->M2, a->cur2, {{a->base, a->base2}, {a->prev, a->prev2}, {a->out_res, a->out_res2}})) return rc;
    if (!launch_residual_diff(a, (hipStream_t)stream)) return row_class_unsupported(op, a->C);
    return hip_check(hipGetLastError(), "svdq_residual_diff launch");
}
