// svdq_residual_diff: the decision pass of First-Block Cache (reference: nunchaku/caching/utils_v2.py:133,176 `hidden - original`,
// fbcache.py:275-277 `(t1 - t2).abs().mean() / t1.abs().mean()` -- six torch launches over the image stream there, one pass here).
//
//   r = base ? round16(cur - base) : cur;   out_res = r (if given);
//   sum_diff += |round16(prev - r)|;   sum_prev += |prev|        (if prev is given)
//
// HBM-bound: 3 reads + 1 write of 2 bytes per element.  One wave per row with the whole row in registers, as residual_kernel.
// The two sums are bit-reproducible: no floating-point atomics.  Every lane adds its own elements in index order, a 6-level butterfly
// folds the wave, the row's pair goes to `partials`; a second one-workgroup kernel behind it on the same stream adds the rows in a
// fixed order (thread t: rows t, t + 256, ... in sequence; an 8-level tree over the 256 threads) and derives the 16-bit means and
// their quotient.  A term therefore passes through at most  8 * ceil(C / 512) + 6 + ceil(rows / 256) + 8  additions.
#include "svdq_common.h"

namespace svdq {

template <int DT, int NV /* 16-byte pieces per lane */>
__global__ __launch_bounds__(256) void residual_diff_kernel(const uint16_t *cur, const uint16_t *base, const uint16_t *prev, uint16_t *out,
                                                             int M, int C, int ld, const uint16_t *cur2, const uint16_t *base2,
                                                             const uint16_t *prev2, uint16_t *out2, int M2, float *__restrict__ partials) {
    using T = typename Half<DT>::T;
    const int lane = threadIdx.x & 63;
    const int grow = blockIdx.x * 4 + (threadIdx.x >> 6); // row of the grouped launch = index of its pair in `partials`
    int row = grow;
    if (row >= M) { // rows beyond the first problem belong to the second one (wave-uniform)
        row -= M;
        if (!cur2 || row >= M2) return;
        cur = cur2; base = base2; prev = prev2; out = out2;
    }
    const size_t off = (size_t)row * ld;
    float sd = 0.f, sp = 0.f;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const int c = (v * 64 + lane) * 8; // a wave instruction covers 1 KiB of the row
        if (c >= C) continue;              // ragged tail of the last pass (C is a multiple of 8, not necessarily of 512)
        u16x8 rv = *reinterpret_cast<const u16x8 *>(cur + off + c);
        if (base) {
            const u16x8 bv = *reinterpret_cast<const u16x8 *>(base + off + c);
#pragma unroll
            for (int e = 0; e < 8; e++) rv[e] = hbits(f2h<T>(h2f(hfrom<T>(rv[e])) - h2f(hfrom<T>(bv[e]))));
        }
        if (prev) {
            const u16x8 pv = *reinterpret_cast<const u16x8 *>(prev + off + c);
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float p = h2f(hfrom<T>(pv[e]));
                sd += fabsf(round16<T>(p - h2f(hfrom<T>(rv[e]))));
                sp += fabsf(p);
            }
        }
        if (out) *reinterpret_cast<u16x8 *>(out + off + c) = rv;
    }
    if (!prev) return;
    fold_wave_pair(sd, sp);
    if (lane == 0) {
        partials[2 * (size_t)grow] = sd;
        partials[2 * (size_t)grow + 1] = sp;
    }
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

template <int DT> static int launch_residual_diff(const svdq_residual_diff_args *p, hipStream_t st) {
    const int rows = p->M + (p->cur2 ? p->M2 : 0);
    dim3 grid((rows + 3) / 4), block(256);
#define SVDQ_DIFF_CASE(NV)                                                                                                      \
    case NV:                                                                                                                    \
        hipLaunchKernelGGL((residual_diff_kernel<DT, NV>), grid, block, 0, st, (const uint16_t *)p->cur, (const uint16_t *)p->base, \
                           (const uint16_t *)p->prev, (uint16_t *)p->out_res, p->M, p->C, p->ld, (const uint16_t *)p->cur2,      \
                           (const uint16_t *)p->base2, (const uint16_t *)p->prev2, (uint16_t *)p->out_res2, p->M2, p->partials);  \
        break;
    switch ((p->C + 511) / 512) {
        SVDQ_DIFF_CASE(1) SVDQ_DIFF_CASE(2) SVDQ_DIFF_CASE(3) SVDQ_DIFF_CASE(4) SVDQ_DIFF_CASE(5) SVDQ_DIFF_CASE(6) SVDQ_DIFF_CASE(7) SVDQ_DIFF_CASE(8)
        SVDQ_DIFF_CASE(12) SVDQ_DIFF_CASE(16) SVDQ_DIFF_CASE(24) SVDQ_DIFF_CASE(32)
    default: return -1;
    }
#undef SVDQ_DIFF_CASE
    if (p->prev) launch_diff_reduce(DT, p->partials, rows, p->C, p->result, st);
    return 0;
}

void launch_diff_reduce(int dtype, const float *partials, int rows, int C, svdq_residual_diff_result *result, hipStream_t st) {
    const float inv_n = 1.0f / ((float)rows * (float)C);
    if (dtype == SVDQ_BF16) hipLaunchKernelGGL((residual_diff_reduce_kernel<SVDQ_BF16>), dim3(1), dim3(256), 0, st, partials, rows, inv_n, result);
    else hipLaunchKernelGGL((residual_diff_reduce_kernel<SVDQ_FP16>), dim3(1), dim3(256), 0, st, partials, rows, inv_n, result);
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_residual_diff(const svdq_residual_diff_args *a, void *stream) {
    if (!a) { set_error("svdq_residual_diff: args is NULL"); return SVDQ_E_INVALID; }
    if (!a->cur) { set_error("svdq_residual_diff: cur is NULL"); return SVDQ_E_INVALID; }
    if (!a->out_res && !a->prev) { set_error("svdq_residual_diff: one of out_res / prev is required"); return SVDQ_E_INVALID; }
    if (a->out_res && !a->base) { set_error("svdq_residual_diff: out_res needs base (without base the residual is cur itself)"); return SVDQ_E_INVALID; }
    if (a->prev && (!a->result || !a->partials)) {
        set_error("svdq_residual_diff: prev needs a result record and the partials buffer ([M + M2, 2] fp32)");
        return SVDQ_E_INVALID;
    }
    if (a->M <= 0 || a->C <= 0 || a->C % 8 || a->ld < a->C || a->ld % 8) {
        set_error("svdq_residual_diff: need M=%d > 0, C=%d a multiple of 8, ld=%d >= C and a multiple of 8", a->M, a->C, a->ld);
        return SVDQ_E_INVALID;
    }
    if (((uintptr_t)a->cur | (uintptr_t)a->base | (uintptr_t)a->prev | (uintptr_t)a->out_res) & 15 || ((uintptr_t)a->partials & 7) ||
        ((uintptr_t)a->result & 7)) {
        set_error("svdq_residual_diff: tensors must be 16-byte aligned (partials and result 8-byte)");
        return SVDQ_E_INVALID;
    }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("svdq_residual_diff: unknown dtype %d", a->dtype); return SVDQ_E_INVALID; }
    if (a->cur2) {
        if (a->M2 <= 0 || (a->base != nullptr) != (a->base2 != nullptr) || (a->prev != nullptr) != (a->prev2 != nullptr) ||
            (a->out_res != nullptr) != (a->out_res2 != nullptr)) {
            set_error("svdq_residual_diff: the second problem must mirror the first (and M2 > 0)");
            return SVDQ_E_INVALID;
        }
        if (((uintptr_t)a->cur2 | (uintptr_t)a->base2 | (uintptr_t)a->prev2 | (uintptr_t)a->out_res2) & 15) {
            set_error("svdq_residual_diff: second problem: tensors must be 16-byte aligned");
            return SVDQ_E_INVALID;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const int rc = a->dtype == SVDQ_BF16 ? launch_residual_diff<SVDQ_BF16>(a, st) : launch_residual_diff<SVDQ_FP16>(a, st);
    if (rc) { set_error("svdq_residual_diff: C=%d: ceil(C/512) must be one of {1..8, 12, 16, 24, 32}", a->C); return SVDQ_E_UNSUPPORTED; }
    return hip_check(hipGetLastError(), "svdq_residual_diff launch");
}
