// svdq_gemm_mxfp4: block-scaled FP4 x FP4 GEMM with the plain epilogue.
//
//   out[m, n] = round16( sum_blocks 2^(sa - 127) 2^(sw - 127) sum_{k in block} a[m, k] w[n, k]  +  sum_r round16(lora_act[m, r] * lora_scales[r / 16]) lora_up[n, r]  +  bias[n] )
//
// Both operands are e2m1 codes in natural rows ([rows][K / 2] bytes) with one E8M0 byte per 32 channels, and both scales go to
// v_mfma_scale_f32_32x32x64_f8f6f4 as block exponents: lane (r, h) of an operand holds the 16 bytes of ONE 32-channel block of row r, so its
// scale byte is that block's.  The K loop therefore holds nothing but LDS reads and MFMAs -- no scale MFMA, no per-group v_fmac.
//
// Workgroup: 256 x 128 outputs, 4 waves of 64 x 128 (2 x 4 accumulator tiles of 32 x 32, 128 fp32 registers), one K-step = 128 channels = 64 bytes
// a row.  Staging: a K-step of both operands, 16 KiB + 8 KiB, comes by global-to-LDS DMA (16 bytes a lane: four neighbouring lanes fetch the 64
// contiguous bytes of one row) into one of two buffers; the 16-byte block c of row q sits at q * 64 + ((c ^ ((q >> 2) & 3)) << 4), which makes
// the fragment reads (32 rows x one block per half-wave) conflict-free over 64 banks.  One barrier per K-step: behind it the step's data is
// visible and the other buffer is free, so the next step's DMA is issued before this step's MFMAs.  The scales of a K-step are ONE dword per
// row (four blocks), loaded a step ahead into registers: 2 + 4 dwords a lane; lanes of the upper half shift theirs by a byte, op_sel = 2 ks picks the block.
// Accumulation is fp32 in ascending K inside one workgroup: no split-K, no atomics, two launches are bit-equal.
//
// svdq_gemm_mxfp4_gelu_quant: the same loop (gemm_mxfp4_loop.inc) under the GELU_QUANT epilogue -- GELU, the MXFP4 requantisation for the next
// layer and that layer's low-rank down projection (gemm_mxfp4_gelu_quant_kernel below).
#include <type_traits>

#include "mxfp4_block.h"

namespace svdq {

typedef __attribute__((address_space(3))) uint8_t mx_lds_u8;
typedef __attribute__((address_space(3))) void mx_lds_void;
typedef __attribute__((address_space(3))) v4i mx_lds_v4i;

constexpr int MX_TM = 256, MX_TN = 128;
constexpr int MX_A_BYTES = MX_TM * 64, MX_B_BYTES = MX_TN * 64, MX_STAGE = MX_A_BYTES + MX_B_BYTES; // 24 KiB a stage, 48 KiB a workgroup
constexpr int MX_MAX_LORA_TILES = 16;

struct Mxfp4GemmParams {
    const uint8_t *act, *wgt;
    const uint32_t *ascales, *wscales;
    const void *bias, *lora_up;
    const float *lora_act;
    void *out;
    long long ldo;
    int M, M_pad, N, K, R;
    float lora_scales[MX_MAX_LORA_TILES];
};

template <int DT>
__global__ __launch_bounds__(256, 2) void gemm_mxfp4_kernel(Mxfp4GemmParams p) {
    using T = typename Half<DT>::T;
    using V8 = typename Half<DT>::V8;
#include "gemm_mxfp4_loop.inc"
    // bias in fp32, one rounding, 8-byte stores: accumulator element i of lane (r, h) is column 32 ni + 8 (i >> 2) + 4 h + (i & 3) of row r.  Rows >= M are cut here
#pragma unroll
    for (int mi = 0; mi < 2; mi++) {
        const int m = m0 + wave * 64 + mi * 32 + r;
        if (m >= p.M) continue;
        T *orow = (T *)p.out + (size_t)m * p.ldo;
#pragma unroll
        for (int ni = 0; ni < 4; ni++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int n = n0 + ni * 32 + g * 8 + 4 * h;
                u16x4 bb = {0, 0, 0, 0}, o;
                if (p.bias) bb = *reinterpret_cast<const u16x4 *>((const T *)p.bias + n);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float v = acc[ni][mi][4 * g + e];
                    if (p.bias) v += h2f(hfrom<T>(bb[e]));
                    o[e] = hbits(f2h<T>(v));
                }
                *reinterpret_cast<u16x4 *>(orow + n) = o;
            }
    }
}

// ---- the GELU_QUANT variant: fc1 of an MLP.  Same loop, same low-rank-up MFMAs, and an epilogue that hands fc2 its operands:
//   g = round16(gelu_tanh(acc + bias))              (one rounding; rows >= M: 0)            -> out (OUT16), 16-bit
//   the MXFP4 block quantiser on round16(g * rcp(smooth_next))                               -> qout [M_pad][N / 2], oscales [N / 128][M_pad] dwords
//   lora_act_out[m, :] += g[m, n0 .. n0 + 127] @ down_next[n0 .. n0 + 127, :]                (fp32 atomics, the last thing issued)
// The accumulator tile IS the block quantiser's register layout (mxfp4_block.h): tile ni of a lane is 16 values of the 32-column block ni of its
// row, and the workgroup's 128 columns are one K-step of fc2 -- 64 code bytes and one scale dword a row.  Blocks are walked ni-outermost so that
// the bias and the 16 reciprocals of a block are formed once for both row tiles; g is kept packed, two 16-bit values a register -- the A operand
// of the low-rank MFMAs behind as it stands -- so every finished block frees half its accumulator registers.  The grid covers M_pad rows, so the padding rows of qout / oscales are written (as zeros) too.
struct Mxfp4GeluQuantParams : Mxfp4GemmParams {
    const void *smooth_next, *down_next; // [N] 16-bit or null; rank-major [R_next][N] 16-bit
    uint8_t *qout;
    uint32_t *oscales;
    float *lora_act_out; // [M_pad][R_next], zero before the launch
    int R_next;
};

template <int DT, bool OUT16>
__global__ __launch_bounds__(256, 2) void gemm_mxfp4_gelu_quant_kernel(Mxfp4GeluQuantParams p) {
    using T = typename Half<DT>::T;
    using V8 = typename Half<DT>::V8;
#include "gemm_mxfp4_loop.inc"
    const int mw0 = m0 + wave * 64; // the wave's rows mw0 + 32 mi + r, all < M_pad
    unsigned gp[4][2][8]; // g, two 16-bit values a register in the accumulator's order: tile ni dies into half its registers as the blocks go by
    unsigned pc[2][4][2], sdw[2] = {0, 0};
    const unsigned short one16 = hbits(f2h<T>(1.0f));
    u16x4 bb[4], sv[4];
#pragma unroll
    for (int g = 0; g < 4; g++) { bb[g] = u16x4{0, 0, 0, 0}; sv[g] = u16x4{one16, one16, one16, one16}; }
    auto load_cols = [&](int ni) { // the 16-bit bias and smooth_next of the lane's 16 columns of block ni
        const int nb = n0 + ni * 32 + 4 * h;
        if (p.bias) {
#pragma unroll
            for (int g = 0; g < 4; g++) bb[g] = *reinterpret_cast<const u16x4 *>((const T *)p.bias + nb + 8 * g);
        }
        if (p.smooth_next) {
#pragma unroll
            for (int g = 0; g < 4; g++) sv[g] = *reinterpret_cast<const u16x4 *>((const T *)p.smooth_next + nb + 8 * g);
        }
    };
    load_cols(0);
#pragma unroll
    for (int ni = 0; ni < 4; ni++) {
        // bias and 1 / smooth_next of the lane's 16 columns of block ni.  Without a bias: + 0; without smoothing: rcp(1) = 1 exactly and g * 1 = g,
        // the quantiser's un-smoothed path
        float bs[16], rs[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            bs[i] = h2f(hfrom<T>(bb[i >> 2][i & 3]));
            rs[i] = __builtin_amdgcn_rcpf(h2f(hfrom<T>(sv[i >> 2][i & 3])));
        }
        if (ni + 1 < 4) load_cols(ni + 1); // the next block's, under this block's arithmetic ...
        asm volatile("" ::: "memory");     // ... and no further ahead: hoisted to the top, the four blocks' vectors are 64 registers and g spills
#pragma unroll
        for (int mi = 0; mi < 2; mi++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[ni][mi][i] += bs[i]; // h32 (the bias registers die here)
#pragma unroll
        for (int mi = 0; mi < 2; mi++) {
            const bool live = mw0 + mi * 32 + r < p.M; // a padding row holds gelu(bias): cut to zero, as the quantiser leaves it
            float v[16], amax = 0.f;
#pragma unroll
            for (int i = 0; i < 16; i += 2) {
                f32x2_t t = round16_pair<T>(gelu_tanh_f(acc[ni][mi][i]), gelu_tanh_f(acc[ni][mi][i + 1]));
                if (!live) t = f32x2_t{0.f, 0.f};
                gp[ni][mi][i >> 1] = (unsigned)hbits(f2h<T>(t[0])) | (unsigned)hbits(f2h<T>(t[1])) << 16; // (exact: t is a 16-bit value)
                asm volatile("" : "+v"(gp[ni][mi][i >> 1])); // (pinned here: sunk to its use behind the blocks, the pack keeps both fp32 values alive and they spill)
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    v[i + e] = smooth_div16<T>(t[e], rs[i + e]);
                    amax = mx_amax_acc(amax, v[i + e]);
                }
            }
            const unsigned sb = mx_block_byte<T>(amax);
            MX_BLOCK_CODES(v, sb, pc[mi][ni]);
            sdw[mi] |= sb << (8 * ni);
            if constexpr (OUT16) {
                if (live) {
                    T *orow = (T *)p.out + (size_t)(mw0 + mi * 32 + r) * p.ldo + n0 + ni * 32 + 4 * h;
#pragma unroll
                    for (int g = 0; g < 4; g++) *reinterpret_cast<uint2 *>(orow + 8 * g) = make_uint2(gp[ni][mi][2 * g], gp[ni][mi][2 * g + 1]);
                }
            }
            __builtin_amdgcn_sched_barrier(0); // one (block, row tile) at a time: interleaved, the values of several are live at once and g spills
        }
    }
    // the row's 64 code bytes of this K-step: 32 contiguous bytes a lane; half 0 stores the row's scale dword
#pragma unroll
    for (int mi = 0; mi < 2; mi++) {
        const int m = mw0 + mi * 32 + r;
        unsigned dw[8];
        mx_trade_halves(pc[mi], h, dw);
        uint8_t *dst = p.qout + (size_t)m * (p.N / 2) + bn * 64 + 32 * h;
        *reinterpret_cast<uint4 *>(dst) = make_uint4(dw[0], dw[1], dw[2], dw[3]);
        *reinterpret_cast<uint4 *>(dst + 16) = make_uint4(dw[4], dw[5], dw[6], dw[7]);
        if (h == 0) p.oscales[(size_t)bn * p.M_pad + m] = sdw[mi];
    }
    // fc2's low-rank down projection on the un-smoothed g, 32 ranks a pass on the 16-bit 32x32x16 MFMA.  A lane's elements 8 q .. 8 q + 7
    // of tile ni -- columns 32 ni + 16 q + 8 (j >> 2) + 4 h + (j & 3) of its row -- are k-slots 8 h + j of the A operand as they stand; the B operand
    // is gathered from the rank-major image in the same order (lane (r, h): rank t2 + r), so the contraction index is permuted on both sides alike.
    // D has the rank along the lanes: an atomic instruction hits 4 rows x 128 contiguous bytes.  The atomics come last (vmcnt retires in order and
    // counts them): nothing waits behind them.  Row tiles entirely in the padding contribute nothing and are skipped.
    const int mws = m0 + __builtin_amdgcn_readfirstlane(wave) * 64; // = mw0, as a scalar
    for (int t2 = 0; t2 < p.R_next; t2 += 32) {
        const bool rank_live = t2 + r < p.R_next; // a half-filled 32-rank tile: zeros beyond R_next
        V8 wv[4][2];
#pragma unroll
        for (int ni = 0; ni < 4; ni++)
#pragma unroll
            for (int q = 0; q < 2; q++) {
                u16x4 w0 = {0, 0, 0, 0}, w1 = {0, 0, 0, 0};
                if (rank_live) {
                    const T *src = (const T *)p.down_next + (size_t)(t2 + r) * p.N + n0 + ni * 32 + q * 16 + 4 * h;
                    w0 = *reinterpret_cast<const u16x4 *>(src);
                    w1 = *reinterpret_cast<const u16x4 *>(src + 8);
                }
#pragma unroll
                for (int j = 0; j < 4; j++) { wv[ni][q][j] = hfrom<T>(w0[j]); wv[ni][q][4 + j] = hfrom<T>(w1[j]); }
            }
        v16f d[2];
#pragma unroll
        for (int mi = 0; mi < 2; mi++)
#pragma unroll
            for (int i = 0; i < 16; i++) d[mi][i] = 0.f;
#pragma unroll
        for (int ni = 0; ni < 4; ni++)
#pragma unroll
            for (int q = 0; q < 2; q++)
#pragma unroll
                for (int mi = 0; mi < 2; mi++) {
                    const V8 gv = __builtin_bit_cast(V8, v4i{(int)gp[ni][mi][4 * q], (int)gp[ni][mi][4 * q + 1], (int)gp[ni][mi][4 * q + 2], (int)gp[ni][mi][4 * q + 3]});
                    d[mi] = Half<DT>::mfma32(gv, wv[ni][q], d[mi]);
                }
#pragma unroll
        for (int mi = 0; mi < 2; mi++) {
            if (!rank_live || mws + mi * 32 >= p.M) continue;
            // D element i: row (i & 3) + 8 (i >> 2) + 4 h, column (rank) r.  A uniform row base (from the scalar wave index) + one 32-bit lane offset:
            // the 16 atomics take the saddr form, no 64-bit address a lane
            float *base = p.lora_act_out + (size_t)(mws + mi * 32) * p.R_next;
            const unsigned off = (unsigned)(4 * h * p.R_next + t2 + r);
#pragma unroll
            for (int i = 0; i < 16; i++) unsafeAtomicAdd(base + (size_t)((i & 3) + 8 * (i >> 2)) * p.R_next + off, d[mi][i]);
        }
    }
}

// clears lora_act_out ahead of the GELU_QUANT launch (a kernel, not hipMemsetAsync: the launch may be recorded into a graph)
static __global__ __launch_bounds__(256) void gemm_mxfp4_clear(uint32_t *dst, size_t words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) dst[i] = 0u;
}

} // namespace svdq

using namespace svdq;

// what both entries check of the fields they share (A: svdq_gemm_mxfp4_args or svdq_gemm_mxfp4_gelu_quant_args); 0 or the error code, nothing is launched.
// `rows`: the rows the grid covers.  fills the kernel's parameters
template <typename A> static int mx_gemm_validate(const A *a, const char *fn, bool need_out, int rows, Mxfp4GemmParams &p, long long &grid) {
    if (!a) { set_error("%s: args is NULL", fn); return SVDQ_E_INVALID; }
    if (!a->act || !a->wgt || !a->ascales || !a->wscales || (need_out && !a->out)) {
        set_error("%s: act, wgt, ascales, wscales%s are required", fn, need_out ? " and out" : ", qout and oscales");
        return SVDQ_E_INVALID;
    }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("%s: unknown dtype %d", fn, a->dtype); return SVDQ_E_INVALID; }
    if (a->M <= 0 || a->M_pad < a->M || a->M_pad % 256) {
        set_error("%s: need 0 < M=%d <= M_pad=%d and M_pad %% 256 == 0", fn, a->M, a->M_pad);
        return SVDQ_E_INVALID;
    }
    if (a->N <= 0 || a->N % 128) { set_error("%s: N=%d must be a positive multiple of 128", fn, a->N); return SVDQ_E_INVALID; }
    if (a->K <= 0 || a->K % 128) { set_error("%s: K=%d must be a positive multiple of 128", fn, a->K); return SVDQ_E_INVALID; }
    if (a->out && (a->ldo < a->N || a->ldo % 4)) { set_error("%s: ldo=%d must be >= N and a multiple of 4", fn, a->ldo); return SVDQ_E_INVALID; }
    if (a->R < 0 || a->R % 16 || a->R > 16 * MX_MAX_LORA_TILES) { set_error("%s: R=%d must be a multiple of 16 in [0, 256]", fn, a->R); return SVDQ_E_INVALID; }
    if (a->R > 0 && (!a->lora_act_in || !a->lora_up)) { set_error("%s: R > 0 needs lora_act_in and lora_up", fn); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->act | (uintptr_t)a->wgt | (uintptr_t)a->lora_act_in | (uintptr_t)a->lora_up) & 15) {
        set_error("%s: act, wgt, lora_act_in and lora_up must be 16-byte aligned", fn);
        return SVDQ_E_INVALID;
    }
    if (((uintptr_t)a->out | (uintptr_t)a->bias) & 7) { set_error("%s: out and bias must be 8-byte aligned", fn); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->ascales | (uintptr_t)a->wscales) & 3) { set_error("%s: ascales and wscales must be 4-byte aligned", fn); return SVDQ_E_INVALID; }
    // addressing reach: the operand tiles are fetched through buffer descriptors with 32-bit byte offsets
    if ((long long)a->M_pad * (a->K / 2) > 0x7fffffffLL || (long long)a->N * (a->K / 2) > 0x7fffffffLL) {
        set_error("%s: M_pad * K / 2 = %lld or N * K / 2 = %lld bytes exceed the 2147483647 the tile loads reach", fn, (long long)a->M_pad * (a->K / 2),
                  (long long)a->N * (a->K / 2));
        return SVDQ_E_UNSUPPORTED;
    }
    grid = (long long)((rows + MX_TM - 1) / MX_TM) * (a->N / MX_TN);
    if (grid > 0x7fffffffLL) { set_error("%s: M=%d x N=%d needs more than 2147483647 workgroups", fn, rows, a->N); return SVDQ_E_UNSUPPORTED; }
    p = Mxfp4GemmParams{(const uint8_t *)a->act, (const uint8_t *)a->wgt, (const uint32_t *)a->ascales, (const uint32_t *)a->wscales, a->bias, a->lora_up,
                        (const float *)a->lora_act_in, a->out, a->ldo, a->M, a->M_pad, a->N, a->K, a->R, {}};
    for (int i = 0; i < MX_MAX_LORA_TILES; i++) p.lora_scales[i] = (a->lora_scales && i < a->R / 16) ? a->lora_scales[i] : 1.0f;
    return 0;
}

extern "C" int svdq_gemm_mxfp4(const svdq_gemm_mxfp4_args *a, void *stream) {
    Mxfp4GemmParams p;
    long long grid;
    if (const int rc = mx_gemm_validate(a, "svdq_gemm_mxfp4", true, a ? a->M : 0, p, grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == SVDQ_BF16) hipLaunchKernelGGL((gemm_mxfp4_kernel<SVDQ_BF16>), dim3((unsigned)grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((gemm_mxfp4_kernel<SVDQ_FP16>), dim3((unsigned)grid), dim3(256), 0, st, p);
    return hip_check(hipGetLastError(), "svdq_gemm_mxfp4 launch");
}

extern "C" int svdq_gemm_mxfp4_gelu_quant(const svdq_gemm_mxfp4_gelu_quant_args *a, void *stream) {
    const char *fn = "svdq_gemm_mxfp4_gelu_quant";
    Mxfp4GeluQuantParams p;
    long long grid;
    if (const int rc = mx_gemm_validate(a, fn, false, a ? a->M_pad : 0, p, grid)) return rc;
    if (!a->qout || !a->oscales) { set_error("%s: qout and oscales are required", fn); return SVDQ_E_INVALID; }
    if (a->R_next < 0 || a->R_next % 16 || a->R_next > 256) { set_error("%s: R_next=%d must be a multiple of 16 in [0, 256]", fn, a->R_next); return SVDQ_E_INVALID; }
    if (!a->lora_down != !a->lora_act_out) { set_error("%s: lora_down and lora_act_out come together or not at all", fn); return SVDQ_E_INVALID; }
    if ((a->R_next > 0) != (a->lora_down != nullptr)) { set_error("%s: R_next=%d %s lora_down and lora_act_out", fn, a->R_next, a->R_next ? "needs" : "takes no"); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->qout | (uintptr_t)a->lora_down) & 15) { set_error("%s: qout and lora_down must be 16-byte aligned", fn); return SVDQ_E_INVALID; }
    if ((uintptr_t)a->smooth_next & 7) { set_error("%s: smooth_next must be 8-byte aligned", fn); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->oscales | (uintptr_t)a->lora_act_out) & 3) { set_error("%s: oscales and lora_act_out must be 4-byte aligned", fn); return SVDQ_E_INVALID; }
    // (addressing reach of the outputs: every row address is formed in 64 bits -- nothing beyond what the shared checks hold)
    p.smooth_next = a->smooth_next; p.down_next = a->lora_down; p.qout = (uint8_t *)a->qout; p.oscales = (uint32_t *)a->oscales;
    p.lora_act_out = (float *)a->lora_act_out; p.R_next = a->R_next;
    hipStream_t st = (hipStream_t)stream;
    if (a->R_next > 0 && !a->lora_act_zeroed) {
        const size_t words = (size_t)a->M_pad * a->R_next, blocks = (words + 1023) / 1024;
        hipLaunchKernelGGL(gemm_mxfp4_clear, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, (uint32_t *)a->lora_act_out, words);
    }
    const dim3 g((unsigned)grid), b(256);
    if (a->dtype == SVDQ_BF16) {
        if (a->out) hipLaunchKernelGGL((gemm_mxfp4_gelu_quant_kernel<SVDQ_BF16, true>), g, b, 0, st, p);
        else hipLaunchKernelGGL((gemm_mxfp4_gelu_quant_kernel<SVDQ_BF16, false>), g, b, 0, st, p);
    } else {
        if (a->out) hipLaunchKernelGGL((gemm_mxfp4_gelu_quant_kernel<SVDQ_FP16, true>), g, b, 0, st, p);
        else hipLaunchKernelGGL((gemm_mxfp4_gelu_quant_kernel<SVDQ_FP16, false>), g, b, 0, st, p);
    }
    return hip_check(hipGetLastError(), "svdq_gemm_mxfp4_gelu_quant launch");
}
