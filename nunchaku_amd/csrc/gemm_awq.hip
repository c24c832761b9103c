// svdq_gemm_awq: AWQ W4A16 GEMM (group 128) for the 4-bit T5 text encoder's projections.
// Reference: ops.gemm_awq (nunchaku/csrc/ops.h:148-160 -> src/kernels/awq/gemm_awq.cu), module
// nunchaku/models/text_encoders/linear.py (W4Linear), weight format text_encoders/tinychat_utils.py (pack_w4).
//
// Contract (the reference's rounding points, gemm_awq.cu:352-358 + MMA):
//   w16[n,k] = round16(fma(q[n,k], scales[k/128, n], scaled_zeros[k/128, n]))    one 16-bit rounding (__hfma2)
//   out[m,n] = round16(sum_k w16[n,k] * x[m,k])                                  exact products, fp32 sums (MFMA)
//   (+ bias[n]: one more 16-bit rounding, W4Linear.forward's `out + bias`)
//
// Structure (DESIGN.md "AWQ GEMM"): a workgroup of 4 waves owns a BM x 128 output tile and walks K in steps of 128 = one
// quantisation group, so every thread needs ONE scale and ONE zero per step.  Per step the workgroup
//   * stages x [BM x 128] as stored into LDS, and
//   * dequantises the step's 128 x 128 codes cooperatively ONCE into a 16-bit B image in LDS (64 weights per thread),
// then each wave runs its (BM / WM) x (128 / WN) sub-tile on v_mfma_f32_32x32x16_{bf16,f16}: a dequantised weight feeds
// BM rows of MFMA work, not one wave's.  The next step's global loads are issued before the MFMAs of the current one
// (register prefetch); two workgroups per CU let one's dequantisation run beside the other's MFMAs.
// K-split: blockIdx.z is a slice of the K-steps; with splits > 1 every slice stores its fp32 tile into the workspace and
// gemm_awq_reduce_kernel adds the slices in slice order (fixed: bit-identical from launch to launch), rounds and adds bias.
// No workgroup waits for another.
#include "svdq_common.h"

namespace svdq {

constexpr int AWQ_GEMM_GROUP = 128; // quantisation group = K-step
constexpr int AWQ_BN = 128;         // output channels per tile
constexpr int AWQ_ROW = 136;        // 16-bit elements per LDS row: 128 + 8 (272 B: the 16 lanes of a ds_read_b128 phase hit 16 distinct 16-B slots)
constexpr int AWQ_SLOTS = 256;      // planner: workgroups wanted per launch (one per CU of an MI355X; a fixed number, so the plan -- and with it the
                                    // fp32 summation order -- depends on (M, N, K) only)

typedef float awq_v2f __attribute__((ext_vector_type(2)));
typedef __bf16 awq_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 awq_f16x2 __attribute__((ext_vector_type(2)));

// 16 int16 of the checkpoint (two 16-byte pieces: halves h = 0, 1 of one 64-channel chunk of one output channel) -> 64 16-bit
// weights in channel order, written to LDS as 8 x 16 bytes.  Int16 j of half h holds channels 32h + 8e + j at nibble e
// (tinychat_utils.py pack_w4); dword i of a piece holds int16 2i (low half) and 2i + 1, so the codes of ADJACENT channels
// (8e + 2i, 8e + 2i + 1) sit in one dword at bits 4e and 16 + 4e: every output dword is one pair.
template <int DT> __device__ __forceinline__ void awq_dequant64(uint16_t *dst /* LDS, 64 channels */, const v4i q0, const v4i q1, unsigned sbits,
                                                                unsigned zbits, unsigned magic);

template <>
__device__ __forceinline__ void awq_dequant64<SVDQ_BF16>(uint16_t *dst, const v4i q0, const v4i q1, unsigned sbits, unsigned zbits, unsigned) {
    // nibbles -> f32 through v_cvt_f32_ubyteN on two masked copies of the dword, v_fma_f32 (exact for the checkpoint's scales: q*s has
    // <= 12 significant bits), one v_cvt_pk_bf16_f32 rounds the pair: ~3 VALU per weight
    const float s = h2f(hfrom<__bf16>((uint16_t)sbits)), z = h2f(hfrom<__bf16>((uint16_t)zbits));
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const v4i q = h ? q1 : q0;
        unsigned o[4][4]; // [e][i]
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned w = (unsigned)q[i];
            unsigned ev = w & 0x0f0f0f0fu, od = (w >> 4) & 0x0f0f0f0fu; // byte b: nibble 2*(b&1) (ev) / 2*(b&1)+1 (od) of int16 2i + (b>>1)
            asm volatile("" : "+v"(ev), "+v"(od)); // keep the masks: byte extracts fold into v_cvt_f32_ubyteN instead of v_bfe_u32 + ubyte0
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const unsigned m = (e & 1) ? od : ev;
                const int b = e >> 1;
                const float lo = (float)((m >> (8 * b)) & 0xffu), hi = (float)((m >> (8 * b + 16)) & 0xffu);
                const awq_bf16x2 pk = __builtin_convertvector((awq_v2f){__builtin_fmaf(lo, s, z), __builtin_fmaf(hi, s, z)}, awq_bf16x2);
                o[e][i] = __builtin_bit_cast(unsigned, pk);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; e++)
            *reinterpret_cast<v4i *>(dst + 32 * h + 8 * e) = v4i{(int)o[e][0], (int)o[e][1], (int)o[e][2], (int)o[e][3]};
    }
}

template <>
__device__ __forceinline__ void awq_dequant64<SVDQ_FP16>(uint16_t *dst, const v4i q0, const v4i q1, unsigned sbits, unsigned zbits, unsigned magic) {
    // the packed 16-bit pipe (as the GEMV's M = 1 path): 0x6400 | q is 1024 + q, exact; back to q with one v_pk_add_f16 (nibble at bit 0) or
    // v_pk_fma_f16 (nibble at bit 4: * 1/16 - 64); then v_pk_fma_f16(q, scale, zero) IS the reference's __hfma2: 1.5 VALU per weight
    const awq_f16x2 m1024 = __builtin_bit_cast(awq_f16x2, 0xe400e400u), sixteenth = __builtin_bit_cast(awq_f16x2, 0x2c002c00u),
                    m64 = __builtin_bit_cast(awq_f16x2, 0xd400d400u);
    const awq_f16x2 s2 = __builtin_bit_cast(awq_f16x2, sbits * 0x10001u), z2 = __builtin_bit_cast(awq_f16x2, zbits * 0x10001u);
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const v4i q = h ? q1 : q0;
        unsigned o[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned w = (unsigned)q[i], up = w >> 8;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const unsigned src = e < 2 ? w : up;
                const awq_f16x2 t = __builtin_bit_cast(awq_f16x2, (src & ((e & 1) ? 0x00f000f0u : 0x000f000fu)) | magic);
                const awq_f16x2 qq = (e & 1) ? __builtin_elementwise_fma(t, sixteenth, m64) : t + m1024;
                o[e][i] = __builtin_bit_cast(unsigned, __builtin_elementwise_fma(qq, s2, z2));
            }
        }
#pragma unroll
        for (int e = 0; e < 4; e++)
            *reinterpret_cast<v4i *>(dst + 32 * h + 8 * e) = v4i{(int)o[e][0], (int)o[e][1], (int)o[e][2], (int)o[e][3]};
    }
}

// BM = 32 / 64 / 128 rows per tile; waves WM x WN, each owning a (BM / WM) x (128 / WN) sub-tile of 32 x 32 MFMA tiles
template <int DT, int BM>
__global__ __launch_bounds__(256, 2) void gemm_awq_kernel(const uint16_t *__restrict__ x, const uint8_t *__restrict__ qw,
                                                           const uint16_t *__restrict__ scales, const uint16_t *__restrict__ zeros,
                                                           const uint16_t *__restrict__ bias, uint16_t *__restrict__ out, float *__restrict__ ws,
                                                           int M, int N, int K, int ldx, int tiles_n, int splits) {
    using T = typename Half<DT>::T;
    using V8 = typename Half<DT>::V8;
    constexpr int WM = BM == 128 ? 2 : 1, WN = 4 / WM, TM = BM / WM, TN = AWQ_BN / WN, RM = TM / 32, RN = TN / 32;
    constexpr int XL = BM / 16; // 16-byte x loads per thread and K-step
    __shared__ __attribute__((aligned(16))) uint16_t lds[(BM + AWQ_BN) * AWQ_ROW];
    uint16_t *As = lds, *Bs = lds + BM * AWQ_ROW;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bn = (int)blockIdx.x % tiles_n, bm = (int)blockIdx.x / tiles_n, sl = blockIdx.z;
    const int n0 = bn * AWQ_BN, m0 = bm * BM;
    const int KS = K / AWQ_GEMM_GROUP;
    const int kb0 = (int)((long long)sl * KS / splits), kb1 = (int)((long long)(sl + 1) * KS / splits);

    // code loader: row group qrg of the tile (4 output channels, 2K bytes per row group in HBM), chunk qc (64 channels) of the step, row qr:
    // 32 contiguous bytes = the 16 int16 of one output channel's 64 channels; 8 threads read a row group's 256 bytes of the step
    const int qrg = tid >> 3, qc = (tid >> 2) & 1, qr = tid & 3;
    // rows beyond M read row 0 of x, a row group beyond N (N % 128 == 64) row group 0 / channel 0: they only reach accumulator rows / columns
    // that are never stored
    const bool qlive = n0 + 4 * qrg < N; // N % 4 == 0: a row group is wholly inside or outside
    const int qn = qlive ? n0 + 4 * qrg + qr : 0;
    const uint8_t *qsrc = qw + (qlive ? (size_t)(n0 / 4 + qrg) * K * 2 + qc * 128 + qr * 32 : 0);

    v4i xr[XL], q0, q1;
    unsigned sb, zb;
    auto load = [&](int kb) {
        const int k0 = kb * AWQ_GEMM_GROUP;
#pragma unroll
        for (int i = 0; i < XL; i++) {
            const int p = i * 256 + tid, row = p >> 4, col = p & 15;
            xr[i] = *reinterpret_cast<const v4i *>(x + (size_t)(m0 + row < M ? m0 + row : 0) * ldx + k0 + col * 8);
        }
        q0 = *reinterpret_cast<const v4i *>(qsrc + (size_t)k0 * 2);
        q1 = *reinterpret_cast<const v4i *>(qsrc + (size_t)k0 * 2 + 16);
        sb = scales[(size_t)kb * N + qn];
        zb = zeros[(size_t)kb * N + qn];
    };
    // gfx9 VOP3 takes no literal and one scalar operand: the fp16 path's v_and_or_b32 needs one of its two constants in a VGPR
    unsigned magic = 0x64006400u;
    asm volatile("" : "+v"(magic));

    v16f acc[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; i++)
#pragma unroll
        for (int j = 0; j < RN; j++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[i][j][v] = 0.f;

    const int wm = wave / WN, wn = wave % WN;
    const uint16_t *afrag = As + (wm * TM + (lane & 31)) * AWQ_ROW + 8 * (lane >> 5);
    const uint16_t *bfrag = Bs + (wn * TN + (lane & 31)) * AWQ_ROW + 8 * (lane >> 5);

    if (kb0 < kb1) load(kb0);
    for (int kb = kb0; kb < kb1; kb++) {
        __syncthreads(); // the previous step's fragment reads are done
#pragma unroll
        for (int i = 0; i < XL; i++) {
            const int p = i * 256 + tid, row = p >> 4, col = p & 15;
            *reinterpret_cast<v4i *>(As + row * AWQ_ROW + col * 8) = xr[i];
        }
        awq_dequant64<DT>(Bs + (4 * qrg + qr) * AWQ_ROW + 64 * qc, q0, q1, sb, zb, magic);
        __syncthreads();
        if (kb + 1 < kb1) load(kb + 1); // in flight under this step's MFMAs
#pragma unroll
        for (int kk = 0; kk < AWQ_GEMM_GROUP / 16; kk++) {
            V8 a[RM], b[RN];
#pragma unroll
            for (int i = 0; i < RM; i++) a[i] = *reinterpret_cast<const V8 *>(afrag + i * 32 * AWQ_ROW + kk * 16);
#pragma unroll
            for (int j = 0; j < RN; j++) b[j] = *reinterpret_cast<const V8 *>(bfrag + j * 32 * AWQ_ROW + kk * 16);
#pragma unroll
            for (int i = 0; i < RM; i++)
#pragma unroll
                for (int j = 0; j < RN; j++) acc[i][j] = Half<DT>::mfma32(a[i], b[j], acc[i][j]);
        }
    }

    // accumulator register v of tile (i, j): row (v & 3) + 8 (v >> 2) + 4 (lane >> 5), column lane & 31
#pragma unroll
    for (int i = 0; i < RM; i++)
#pragma unroll
        for (int j = 0; j < RN; j++) {
            const int n = n0 + wn * TN + j * 32 + (lane & 31);
            if (n >= N) continue;
            float bv = 0.f;
            if (splits == 1 && bias) bv = h2f(hfrom<T>(bias[n]));
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int m = m0 + wm * TM + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5);
                if (m >= M) continue;
                if (splits > 1) {
                    ws[((size_t)sl * M + m) * N + n] = acc[i][j][v];
                } else {
                    float y = round16<T>(acc[i][j][v]);
                    if (bias) y = round16<T>(y + bv);
                    out[(size_t)m * N + n] = hbits(f2h<T>(y));
                }
            }
        }
}

// the K-split's second kernel: slices added in slice order, one 16-bit rounding, then the bias as a 16-bit add
template <int DT>
__global__ __launch_bounds__(256) void gemm_awq_reduce_kernel(const float *__restrict__ ws, const uint16_t *__restrict__ bias, uint16_t *__restrict__ out,
                                                               int M, int N, int splits) {
    using T = typename Half<DT>::T;
    const size_t MN = (size_t)M * N, idx = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (idx >= MN) return;
    v4f a = *reinterpret_cast<const v4f *>(ws + idx);
    for (int s = 1; s < splits; s++) a += *reinterpret_cast<const v4f *>(ws + (size_t)s * MN + idx);
    const int n = (int)(idx % N);
    u16x4 o;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        float y = round16<T>(a[t]);
        if (bias) y = round16<T>(y + h2f(hfrom<T>(bias[n + t])));
        o[t] = hbits(f2h<T>(y));
    }
    *reinterpret_cast<u16x4 *>(out + idx) = o;
}

struct AwqPlan { int bm, tiles_m, tiles_n, splits; };

// tile rows from M; K-split (powers of two, >= 4 K-steps per slice, at most 16 slices) until the launch has AWQ_SLOTS workgroups
static AwqPlan awq_plan(int M, int N, int K, bool with_workspace) {
    AwqPlan p;
    p.bm = M <= 32 ? 32 : M <= 64 ? 64 : 128;
    p.tiles_m = (M + p.bm - 1) / p.bm;
    p.tiles_n = (N + AWQ_BN - 1) / AWQ_BN;
    p.splits = 1;
    const int ks = K / AWQ_GEMM_GROUP;
    const long long tiles = (long long)p.tiles_m * p.tiles_n;
    while (with_workspace && tiles * p.splits < AWQ_SLOTS && ks >= 8 * p.splits && p.splits < 16) p.splits *= 2;
    return p;
}

static int64_t awq_workspace_bytes(const AwqPlan &p, int M, int N) { return p.splits > 1 ? (int64_t)p.splits * M * N * 4 : 0; }

template <int DT> static void launch_gemm_awq(const svdq_gemm_awq_args *a, const AwqPlan &p, hipStream_t st) {
    const dim3 grid(p.tiles_m * p.tiles_n, 1, p.splits), block(256);
    const uint16_t *x = (const uint16_t *)a->x, *sc = (const uint16_t *)a->scales, *zr = (const uint16_t *)a->scaled_zeros,
                   *bias = (const uint16_t *)a->bias;
    const uint8_t *qw = (const uint8_t *)a->qweight;
    uint16_t *out = (uint16_t *)a->out;
    float *ws = (float *)a->workspace;
#define SVDQ_AWQ_CASE(BMV)                                                                                                                     \
    case BMV:                                                                                                                                  \
        hipLaunchKernelGGL((gemm_awq_kernel<DT, BMV>), grid, block, 0, st, x, qw, sc, zr, bias, out, ws, a->M, a->N, a->K, a->ldx, p.tiles_n,   \
                           p.splits);                                                                                                          \
        break;
    switch (p.bm) {
        SVDQ_AWQ_CASE(32) SVDQ_AWQ_CASE(64) SVDQ_AWQ_CASE(128)
    }
#undef SVDQ_AWQ_CASE
    if (p.splits > 1) {
        const size_t quads = (size_t)a->M * a->N / 4;
        hipLaunchKernelGGL((gemm_awq_reduce_kernel<DT>), dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, ws, bias, out, a->M, a->N, p.splits);
    }
}

} // namespace svdq

using namespace svdq;

extern "C" int64_t svdq_gemm_awq_workspace_bytes(int32_t M, int32_t N, int32_t K) {
    if (M < 1 || N < 1 || K < AWQ_GEMM_GROUP) return 0;
    return awq_workspace_bytes(awq_plan(M, N, K, true), M, N);
}

extern "C" int svdq_gemm_awq(const svdq_gemm_awq_args *a, void *stream) {
    if (!a) { set_error("svdq_gemm_awq: args is NULL"); return SVDQ_E_INVALID; }
    if (!a->x || !a->qweight || !a->scales || !a->scaled_zeros || !a->out) {
        set_error("svdq_gemm_awq: x, qweight, scales, scaled_zeros and out are required");
        return SVDQ_E_INVALID;
    }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("svdq_gemm_awq: unknown dtype %d", a->dtype); return SVDQ_E_INVALID; }
    if (a->group_size != AWQ_GEMM_GROUP) {
        set_error("svdq_gemm_awq: group_size=%d (only 128 is implemented, as in the reference's gemm_awq)", a->group_size);
        return SVDQ_E_UNSUPPORTED;
    }
    if (a->M < 1) { set_error("svdq_gemm_awq: M=%d must be >= 1", a->M); return SVDQ_E_INVALID; }
    if (a->N <= 0 || a->N % 64) { set_error("svdq_gemm_awq: N=%d must be a positive multiple of 64", a->N); return SVDQ_E_INVALID; }
    if (a->K <= 0 || a->K % AWQ_GEMM_GROUP) { set_error("svdq_gemm_awq: K=%d must be a positive multiple of 128", a->K); return SVDQ_E_INVALID; }
    if (a->ldx < a->K || a->ldx % 8) { set_error("svdq_gemm_awq: ldx=%d must be >= K and a multiple of 8", a->ldx); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->x | (uintptr_t)a->qweight) & 15) { set_error("svdq_gemm_awq: x and qweight must be 16-byte aligned"); return SVDQ_E_INVALID; }
    // (the K-split's reduce kernel stores out in 8-byte pieces of four elements; scales, scaled_zeros and bias are read one element at a time)
    if ((uintptr_t)a->out & 7) { set_error("svdq_gemm_awq: out must be 8-byte aligned"); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->scales | (uintptr_t)a->scaled_zeros | (uintptr_t)a->bias) & 1) { set_error("svdq_gemm_awq: scales, scaled_zeros and bias must be 2-byte aligned"); return SVDQ_E_INVALID; }
    if ((uintptr_t)a->workspace & 15) { set_error("svdq_gemm_awq: workspace must be 16-byte aligned"); return SVDQ_E_INVALID; }
    const AwqPlan p = awq_plan(a->M, a->N, a->K, a->workspace != nullptr);
    const int64_t need = awq_workspace_bytes(p, a->M, a->N);
    if (a->workspace && a->workspace_bytes < need) {
        set_error("svdq_gemm_awq: workspace of %lld bytes; this launch needs %lld (svdq_gemm_awq_workspace_bytes), 16-byte aligned",
                  (long long)a->workspace_bytes, (long long)need);
        return SVDQ_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == SVDQ_BF16) launch_gemm_awq<SVDQ_BF16>(a, p, st);
    else launch_gemm_awq<SVDQ_FP16>(a, p, st);
    return hip_check(hipGetLastError(), "svdq_gemm_awq launch");
}
