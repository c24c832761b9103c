// What the one-wave-per-row kernels share (residual.hip, residual_diff.hip, modulated_diff.hip): the width classes and their dispatch, the
// 16-byte piece access, the grouped launch's row resolution, the tail of a decision pass (the two fp32 sums) and the host-side validation.
//
// A row pass: 256 threads = 4 waves = 4 rows per workgroup; a wave instruction covers 1 KiB of its row (64 lanes x one 16-byte piece of eight
// 16-bit elements), so lane l holds piece v of the row at column  c = (v * 64 + l) * 8,  v = 0 .. NV - 1,  NV = ceil(C / 512) pieces per lane.
// C is a multiple of 8, not necessarily of 512: the lanes with c >= C skip the ragged tail of the last pass.  A kernel keeps its own plain
// `#pragma unroll for (v ...)` loop and calls the helpers from it (a loop wrapped in a functor compiled to longer code with more registers).
#pragma once

#include <initializer_list>
#include <type_traits>
#include <utility>

#include "svdq_common.h"

namespace svdq {

// ---- width classes -------------------------------------------------------------------------------------------------------------------
// NV is a template parameter (the unrolled piece loop, residual_kernel's register-resident row).  This list is the only one: a class outside
// it has no instantiation and its widths are refused (SVDQ_E_UNSUPPORTED), never rounded up to a neighbour.
using RowClasses = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 32>;

template <int DT, typename F, int... NV> bool for_row_class_of(int nv, F &f, std::integer_sequence<int, NV...>) {
    return ((nv == NV && (f(std::integral_constant<int, DT>{}, std::integral_constant<int, NV>{}), true)) || ...);
}
// calls f(integral_constant<DT>, integral_constant<NV>) for the class of C; false (f not called) for a class with no instantiation.
// dtype: SVDQ_BF16 | SVDQ_FP16 (validated by the caller)
template <typename F> bool for_row_class(int dtype, int C, F f) {
    const int nv = (C + 511) / 512;
    return dtype == SVDQ_BF16 ? for_row_class_of<SVDQ_BF16>(nv, f, RowClasses{}) : for_row_class_of<SVDQ_FP16>(nv, f, RowClasses{});
}
inline int row_class_unsupported(const char *op, int C) {
    set_error("%s: C=%d: ceil(C/512) must be one of {1..8, 12, 16, 24, 32}", op, C);
    return SVDQ_E_UNSUPPORTED;
}

// ---- device: pieces and rows ---------------------------------------------------------------------------------------------------------
// one 16-byte piece (16-byte aligned: C, ld and the base pointers are validated on the host)
__device__ __forceinline__ u16x8 ld8(const uint16_t *p) { return *reinterpret_cast<const u16x8 *>(p); }
__device__ __forceinline__ void st8(uint16_t *p, u16x8 v) { *reinterpret_cast<u16x8 *>(p) = v; }

__device__ __forceinline__ int wave_row() { return blockIdx.x * 4 + (threadIdx.x >> 6); }
// grouped launch (two problems of one width in one grid): the rows beyond the first problem's M belong to the second one (wave-uniform).
// For such a row: makes it the row inside the second problem; false = there is no second problem (`lead2`: its first tensor) or no such row
__device__ __forceinline__ bool second_problem_row(int &row, int M, const void *lead2, int M2) {
    row -= M;
    return lead2 && row < M2;
}

// ---- device: the two fp32 sums of a decision pass (residual_diff_kernel, modulated_diff_kernel) -------------------------------------
// One fixed order, no floating-point atomics: every lane adds its own elements in index order (add_distance, piece after piece), a 6-level
// butterfly folds the wave (fold_wave_pair), the row's pair goes to `partials` (store_row_pair); launch_diff_reduce behind it on the same
// stream adds the rows in a fixed order.  A term passes through at most  8 * ceil(C / 512) + 6 + ceil(rows / 256) + 8  additions.
// sd += |round16(prev - m)|, sp += |prev| over the eight elements of one piece
template <typename T> __device__ __forceinline__ void add_distance(u16x8 pv, u16x8 mv, float &sd, float &sp) {
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const float p = h2f(hfrom<T>(pv[e]));
        sd += fabsf(round16<T>(p - h2f(hfrom<T>(mv[e]))));
        sp += fabsf(p);
    }
}
__device__ __forceinline__ void fold_wave_pair(float &sd, float &sp) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sd += __shfl_xor(sd, o); sp += __shfl_xor(sp, o); }
}
// `row`: the row of the launch (of a grouped launch: over both problems) = the index of its pair
__device__ __forceinline__ void store_row_pair(float *__restrict__ partials, int row, int lane, float sd, float sp) {
    fold_wave_pair(sd, sp);
    if (lane == 0) {
        partials[2 * (size_t)row] = sd;
        partials[2 * (size_t)row + 1] = sp;
    }
}
// the finishing stage (residual_diff.hip): one workgroup adds the `rows` pairs of `partials` in a fixed order and fills `result` with the
// sums, the 16-bit means over rows * C terms and their 16-bit quotient.  dtype: SVDQ_BF16 | SVDQ_FP16 (validated by the caller).
void launch_diff_reduce(int dtype, const float *partials, int rows, int C, svdq_residual_diff_result *result, hipStream_t st);

// ---- host: validation ----------------------------------------------------------------------------------------------------------------
inline bool aligned_to(size_t bytes, std::initializer_list<const void *> ptrs) {
    uintptr_t bits = 0;
    for (const void *p : ptrs) bits |= (uintptr_t)p; // (NULL = not given: aligned)
    return !(bits & (bytes - 1));
}
// what every row pass asks of its arguments besides the pointers it requires.  p16: the 16-bit tensors (16-byte pieces), p8: the fp32
// buffers read or written in pairs (stats, partials, the result record).  `op`: the entry point, for the message.  0 or SVDQ_E_INVALID
inline int check_row_args(const char *op, int M, int C, int ld, int dtype, std::initializer_list<const void *> p16,
                          std::initializer_list<const void *> p8) {
    if (M <= 0 || C <= 0 || C % 8 || ld < C || ld % 8) {
        set_error("%s: need M=%d > 0, C=%d a multiple of 8, ld=%d >= C and a multiple of 8", op, M, C, ld);
        return SVDQ_E_INVALID;
    }
    if (!aligned_to(16, p16) || !aligned_to(8, p8)) {
        set_error("%s: 16-bit tensors must be 16-byte aligned, fp32 buffers (stats, partials, result) 8-byte aligned", op);
        return SVDQ_E_INVALID;
    }
    if (dtype != SVDQ_BF16 && dtype != SVDQ_FP16) { set_error("%s: unknown dtype %d", op, dtype); return SVDQ_E_INVALID; }
    return 0;
}
// the second problem of a grouped launch (lead2 = its first tensor, given): M2 rows of the same width, and every optional tensor given
// exactly where the first problem gives it -- the kernel decides what to do from the first problem's pointers
struct MirrorPair { const void *first, *second; };
inline int check_second_problem(const char *op, int M2, const void *lead2, std::initializer_list<MirrorPair> p16,
                                std::initializer_list<MirrorPair> p8 = {}) {
    bool mirrors = M2 > 0, aligned = aligned_to(16, {lead2});
    for (const MirrorPair &p : p16) { mirrors &= (p.first != nullptr) == (p.second != nullptr); aligned &= aligned_to(16, {p.second}); }
    for (const MirrorPair &p : p8) { mirrors &= (p.first != nullptr) == (p.second != nullptr); aligned &= aligned_to(8, {p.second}); }
    if (!mirrors) { set_error("%s: the second problem must mirror the first (and M2 > 0)", op); return SVDQ_E_INVALID; }
    if (!aligned) { set_error("%s: second problem: 16-bit tensors must be 16-byte aligned, fp32 buffers 8-byte aligned", op); return SVDQ_E_INVALID; }
    return 0;
}

} // namespace svdq
