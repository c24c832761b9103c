// svdq_gemv_awq_lora_batched: the low-rank (LoRA) branch of the AWQ W4A16 GEMV, for the AdaLayerNormZero modulation projections.
// Reference: GEMV_AWQ::forward with lora_down / lora_up / lora_scale (src/Linear.cpp): out += lora_scale * (x @ down^T) @ up^T as two
// dense 16-bit GEMMs behind the GEMV.  Here: two launches for ALL layers of a step that carry a LoRA, directly behind
// svdq_gemv_awq_batched on the same stream (nothing is launched when no layer has one).
//
// Rounding points ("Low-rank (LoRA) branch of the GEMV"):
//   t[j]   = round16( sum_k down[j,k] * x[k] )
//   d[n]   = round16( strength * sum_j up[n,j] * t[j] )
//   out[n'] = round16( out[n'] + d[n] )                     n' = (n % c) * (N / c) + n / c for out_chunks = c > 1, else n
// The two sums (and the product with strength) are formed in fp64 and rounded ONCE to 16 bits (round16_f64: fp64 -> fp32 with round-to-odd,
// then the ordinary fp32 -> 16-bit rounding; no double rounding).  An fp32 sum would do for t and d taken alone -- it differs from the exact
// sum only across a rounding boundary -- but a d that is one step off is a step of d, and where out and d nearly cancel that is several steps
// of out (measured: 1 element in 384 at fp16, rank 128, two steps).  The fp64 sums make every rounding point the correctly rounded one, so the
// result equals a float64 restatement bit for bit; the cost is nothing next to the GEMV in front (128 fp64 fmas per output at most).
// Every t[j] has one owner wave and every out[n'] one owner thread, both with a fixed summation order: no atomics, so the
// result is bit-reproducible from launch to launch and does not depend on how the entries are batched.
//
// Phase 1 (down): one wave per (entry, rank j).  The wave walks down[j, :] and x with 16-byte loads per lane (512 input channels per
//   wave instruction), two fp64 chains per lane, then the wave64 butterfly of gemv_awq.hip.
// Phase 2 (up): one thread per output channel; the block stages t as fp32 in LDS (exact), a thread reads its up row ([r] 16-bit, contiguous)
//   with 16-byte loads.  r <= 128: at most 16 loads and 128 fmas per thread.
// The work is tiny next to the GEMV it follows (FLUX.1, r = 16: 7 MB of `down` + 45 MB of `up` against 1.6 GB of 4-bit codes).
#include "svdq_common.h"

namespace svdq {

constexpr int LORA_R_MAX = 128;

// fp64 -> 16 bits in one rounding: to fp32 with round-to-odd (the inexact fp32 neighbour with an odd last bit keeps "above / below / on a tie" visible
// to the next rounding; fp32 has more than 2 x 11 + 2 significant bits), then fp32 -> 16-bit to nearest even
template <typename T> __device__ __forceinline__ float round16_f64(double v) {
    float f = (float)v; // to nearest even
    const double back = (double)f;
    if (back != v && !(__builtin_isinf(f))) {
        unsigned u = __builtin_bit_cast(unsigned, f);
        if (!(u & 1u)) u += (__builtin_fabs(back) < __builtin_fabs(v)) ? 1u : 0xffffffffu; // sign-magnitude: + 1 is away from zero
        f = __builtin_bit_cast(float, u);
    }
    return round16<T>(f);
}

// the descriptors travel in the kernel arguments; a block finds its entry by a scalar scan (as gemv_awq_batched_kernel)
struct LoraDownEntry { const uint16_t *down; uint16_t *t; int r, pad; };
struct LoraDownBatch { LoraDownEntry e[SVDQ_GEMV_BATCH_MAX]; int count; }; // 80 x 24 B + 4
struct LoraUpEntry { const uint16_t *up; const uint16_t *t; uint16_t *out; float strength; int r, N, ochunks; };
struct LoraUpBatch { LoraUpEntry e[SVDQ_GEMV_BATCH_MAX]; int count; }; // 80 x 40 B + 4: under the 4 KiB kernel-argument limit

template <int DT>
__global__ __launch_bounds__(256) void gemv_lora_down_kernel(const uint16_t *__restrict__ x, const LoraDownBatch b, int K) {
    using T = typename Half<DT>::T;
    int i = 0, first = 0; // block-uniform scan: entry i owns blocks [first, first + r_i / 4): four ranks (waves) per block
    while (i + 1 < b.count && (int)blockIdx.x >= first + b.e[i].r / 4) { first += b.e[i].r / 4; i++; }
    const LoraDownEntry &e = b.e[i];
    const int lane = threadIdx.x & 63;
    const int j = ((int)blockIdx.x - first) * 4 + (threadIdx.x >> 6);
    if (j >= e.r) return; // (r % 16 == 0: never taken; keeps the row index in bounds whatever the host passes)
    const uint16_t *row = e.down + (size_t)j * K;
    double acc = 0.0, acc2 = 0.0;
    for (int k = lane * 8; k < K; k += 64 * 8) { // K % 8 == 0: a lane's 8 channels are inside the row
        const u16x8 dv = *reinterpret_cast<const u16x8 *>(row + k);
        const u16x8 xv = *reinterpret_cast<const u16x8 *>(x + k);
#pragma unroll
        for (int v = 0; v < 8; v += 2) {
            acc = __builtin_fma((double)h2f(hfrom<T>(dv[v])), (double)h2f(hfrom<T>(xv[v])), acc);
            acc2 = __builtin_fma((double)h2f(hfrom<T>(dv[v + 1])), (double)h2f(hfrom<T>(xv[v + 1])), acc2);
        }
    }
    double a = acc + acc2;
    a += __shfl_xor(a, 32);
    a += __shfl_xor(a, 16);
    a += __shfl_xor(a, 8);
    a += __shfl_xor(a, 4);
    a += __shfl_xor(a, 2);
    a += __shfl_xor(a, 1);
    if (lane == 0) e.t[j] = hbits(f2h<T>(round16_f64<T>(a)));
}

template <int DT>
__global__ __launch_bounds__(256) void gemv_lora_up_kernel(const LoraUpBatch b) {
    using T = typename Half<DT>::T;
    int i = 0, first = 0; // entry i owns blocks [first, first + ceil(N_i / 256))
    while (i + 1 < b.count && (int)blockIdx.x >= first + (b.e[i].N + 255) / 256) { first += (b.e[i].N + 255) / 256; i++; }
    const LoraUpEntry &e = b.e[i];
    __shared__ __attribute__((aligned(16))) float ts[LORA_R_MAX];
    if ((int)threadIdx.x < e.r) ts[threadIdx.x] = h2f(hfrom<T>(e.t[threadIdx.x]));
    __syncthreads();
    const int n = ((int)blockIdx.x - first) * 256 + (int)threadIdx.x;
    if (n >= e.N) return;
    const uint16_t *row = e.up + (size_t)n * e.r;
    double acc = 0.0;
    for (int j0 = 0; j0 < e.r; j0 += 8) { // r % 16 == 0 and `up` 16-byte aligned: every row piece is an aligned 16-byte load
        const u16x8 uv = *reinterpret_cast<const u16x8 *>(row + j0);
        const v4f t0 = *reinterpret_cast<const v4f *>(ts + j0), t1 = *reinterpret_cast<const v4f *>(ts + j0 + 4);
#pragma unroll
        for (int v = 0; v < 4; v++) acc = __builtin_fma((double)h2f(hfrom<T>(uv[v])), (double)t0[v], acc);
#pragma unroll
        for (int v = 0; v < 4; v++) acc = __builtin_fma((double)h2f(hfrom<T>(uv[4 + v])), (double)t1[v], acc);
    }
    const float d = round16_f64<T>((double)e.strength * acc);
    if (d == 0.f) return; // out + (+-0) is out, except that -0 + +0 would lose its sign: a zero update (strength 0) leaves out bit for bit
    const int no = e.ochunks > 1 ? (n % e.ochunks) * (e.N / e.ochunks) + n / e.ochunks : n; // the GEMV's de-interleaved layout
    e.out[no] = hbits(f2h<T>(h2f(hfrom<T>(e.out[no])) + d));
}

} // namespace svdq

using namespace svdq;

static int validate_gemv_lora(const svdq_gemv_lora_args *a, int i) {
    if (!a->x || !a->down || !a->up || !a->out || !a->t) { set_error("svdq_gemv_awq_lora_batched: entry %d: x, down, up, out and t are required", i); return SVDQ_E_INVALID; }
    if (a->r < 16 || a->r > LORA_R_MAX || a->r % 16) { set_error("svdq_gemv_awq_lora_batched: entry %d: r=%d must be a multiple of 16 in [16, %d]", i, a->r, LORA_R_MAX); return SVDQ_E_INVALID; }
    if (a->N <= 0 || a->K <= 0 || a->K % 8) { set_error("svdq_gemv_awq_lora_batched: entry %d: need N=%d > 0 and K=%d a positive multiple of 8", i, a->N, a->K); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->x | (uintptr_t)a->down | (uintptr_t)a->up) & 15) { set_error("svdq_gemv_awq_lora_batched: entry %d: x, down and up must be 16-byte aligned", i); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->out | (uintptr_t)a->t) & 1) { set_error("svdq_gemv_awq_lora_batched: entry %d: out and t must be 2-byte aligned", i); return SVDQ_E_INVALID; }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("svdq_gemv_awq_lora_batched: entry %d: unknown dtype %d", i, a->dtype); return SVDQ_E_INVALID; }
    if (a->out_chunks < 0 || (a->out_chunks > 1 && a->N % a->out_chunks)) { set_error("svdq_gemv_awq_lora_batched: entry %d: out_chunks=%d must divide N=%d", i, a->out_chunks, a->N); return SVDQ_E_INVALID; }
    return SVDQ_OK;
}

extern "C" int svdq_gemv_awq_lora_batched(const svdq_gemv_lora_args *a, int32_t count, void *stream) {
    if (!a || count < 1 || count > SVDQ_GEMV_BATCH_MAX) { set_error("svdq_gemv_awq_lora_batched: need 1 <= count=%d <= %d entries", count, SVDQ_GEMV_BATCH_MAX); return SVDQ_E_INVALID; }
    LoraDownBatch bd;
    LoraUpBatch bu;
    int blocks_down = 0, blocks_up = 0;
    for (int i = 0; i < count; i++) {
        if (int rc = validate_gemv_lora(a + i, i)) return rc;
        if (a[i].x != a[0].x || a[i].K != a[0].K || a[i].dtype != a[0].dtype) {
            set_error("svdq_gemv_awq_lora_batched: entry %d must share x, K and dtype with entry 0", i);
            return SVDQ_E_INVALID;
        }
        bd.e[i] = LoraDownEntry{(const uint16_t *)a[i].down, (uint16_t *)a[i].t, a[i].r, 0};
        bu.e[i] = LoraUpEntry{(const uint16_t *)a[i].up, (const uint16_t *)a[i].t, (uint16_t *)a[i].out, a[i].strength, a[i].r, a[i].N, a[i].out_chunks};
        blocks_down += a[i].r / 4;
        blocks_up += (a[i].N + 255) / 256;
    }
    bd.count = bu.count = count;
    hipStream_t st = (hipStream_t)stream;
    if (a[0].dtype == SVDQ_BF16) {
        hipLaunchKernelGGL((gemv_lora_down_kernel<SVDQ_BF16>), dim3(blocks_down), dim3(256), 0, st, (const uint16_t *)a[0].x, bd, a[0].K);
        hipLaunchKernelGGL((gemv_lora_up_kernel<SVDQ_BF16>), dim3(blocks_up), dim3(256), 0, st, bu);
    } else {
        hipLaunchKernelGGL((gemv_lora_down_kernel<SVDQ_FP16>), dim3(blocks_down), dim3(256), 0, st, (const uint16_t *)a[0].x, bd, a[0].K);
        hipLaunchKernelGGL((gemv_lora_up_kernel<SVDQ_FP16>), dim3(blocks_up), dim3(256), 0, st, bu);
    }
    return hip_check(hipGetLastError(), "svdq_gemv_awq_lora_batched launch");
}
