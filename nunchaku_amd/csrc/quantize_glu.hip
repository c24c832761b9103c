// svdq_quantize_glu_halves: the W4A4 activation quantiser (quantize.hip) behind a split-half gated activation.
//
//   a = round16(act(float(gate)))      act = silu | erf-gelu, fp32
//   x = round16(float(value) * a)      the 16-bit multiply
// then everything svdq_quantize_w4a4_act_fuse_lora does to x: lora_act += x @ lora_down on the un-smoothed x, smooth_div16, per-(row, 64)
// amax, scale = amax / 7, the FP6 code image and the scale image.  value and gate are two [M, K] 16-bit matrices with their own row strides --
// the two column halves of one [M, 2K] projection output (Z-Image's SwiGLU, SDXL's GEGLU) -- so the 16-bit [M, K] product never exists in HBM.
//
// Design.  The op is HBM-bound: 4 M K bytes in, 0.75 M K out.  A wave owns one F6 chunk (32 rows x 128 channels), a workgroup
// four neighbouring chunks of one row tile, as in quantize_kernel_v2.  What differs is how the chunk comes in:
//   * the activation and the product are element-wise, so both tiles are loaded ROW-CONTIGUOUSLY: 16 lanes x 16 bytes = one 256-byte row, four rows
//     per instruction, 8 + 8 instructions per chunk, all issued before the first is consumed (the record-order loads of the other kernels are
//     8-byte pieces 32 rows apart);
//   * x is computed in that layout and written ONCE, as 16-bit, into the wave's 8 KiB LDS tile (16-byte pieces XOR-swizzled by the row), then
//     read back in record layout (lane = (row, half): 16 ds_read_b64) -- these registers are the quantiser's input AND the A operands of the
//     low-rank MFMAs.  Only a quarter of the loaded bytes make the round trip;
//   * once the tile is back in registers its LDS is dead: the chunk's 32-rank slab of lora_down lands there by LDS-DMA (XOR-swizzled by the
//     rank) while the quantisation proper runs, and the partial sums of the four waves are parked there for the fixed-order combine.  8.5 KiB of
//     LDS per wave keeps four workgroups on a CU.  Ranks above 32 walk the same region slab by slab.
#include "quantize_tail.h"

namespace svdq {

struct GluParams {
    const void *value, *gate, *smooth, *lora_down;
    uint8_t *act;
    void *ascales, *lora_act;
    long long ld_value, ld_gate;
    int M, K, R, mode; // mode: lora_act_add's (bit 0 = K is sliced over workgroups, bit 1 = Q31.32)
};

// (glu_silu, glu_gelu: glu_act.h, shared with the convolution front end and the MXFP4 GEMM's GLU_QUANT epilogue)
template <typename T, int ACT> __device__ __forceinline__ unsigned glu_pair(unsigned vd, unsigned gd) {
    unsigned out = 0;
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const float v = h2f(hfrom<T>((unsigned short)(vd >> (16 * e)))), g = h2f(hfrom<T>((unsigned short)(gd >> (16 * e))));
        const float a = round16<T>(ACT == SVDQ_GLU_SILU ? glu_silu(g) : glu_gelu(g));
        out |= (unsigned)hbits(f2h<T>(v * a)) << (16 * e);
    }
    return out;
}

template <int DT, int ACT, bool SMOOTH>
__global__ __launch_bounds__(256, 3) void quantize_glu_kernel(GluParams p) {
    using T = typename Half<DT>::T;
    using V8 = typename Half<DT>::V8;
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * QG_WAVE_BYTES];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int r = lane & 31, h = lane >> 5;
    const int K = p.K, KP = K / 128;
    const int slices = (KP + 3) / 4;
    const int rt = blockIdx.x / slices, kp = (blockIdx.x % slices) * 4 + wave;
    const bool active = kp < KP; // wave-uniform
    lds_u8 *const W = (lds_u8 *)lds + wave * QG_WAVE_BYTES; // private to the wave until the combine

#define QUANT_TAIL_PART 1 // the record, the slab offsets, slab_dma
#include "quantize_tail.inc"

    if (active) {
        // ---- 1. the chunk's loads, back to back: lane (rr, c16) takes 16 bytes of rows 4i + rr.  A row >= M reads the last row and is zeroed below
        const int c16 = lane & 15, rr = lane >> 4;
        v4i vv[8], gv[8];
        bool live[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int row = rt * 32 + 4 * i + rr;
            live[i] = row < p.M;
            const size_t rowc = (size_t)(live[i] ? row : p.M - 1);
            vv[i] = *reinterpret_cast<const v4i *>((const T *)p.value + rowc * p.ld_value + kp * 128 + 8 * c16);
            gv[i] = *reinterpret_cast<const v4i *>((const T *)p.gate + rowc * p.ld_gate + kp * 128 + 8 * c16);
        }
        unsigned sm2 = 0;
        if constexpr (SMOOTH) sm2 = *reinterpret_cast<const unsigned *>((const T *)p.smooth + kp * 128 + 2 * lane);

        // ---- 2. x in the load layout -> LDS tile, piece c16 of row q at q * 256 + ((c16 ^ (q & 15)) << 4)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            v4i xo;
#pragma unroll
            for (int d = 0; d < 4; d++) xo[d] = live[i] ? (int)glu_pair<T, ACT>((unsigned)vv[i][d], (unsigned)gv[i][d]) : 0;
            const int q = 4 * i + rr;
            *(lds_v4i *)(W + q * 256 + ((c16 ^ (q & 15)) << 4)) = xo;
        }
        if constexpr (SMOOTH) { // lane l: channels 2l, 2l + 1 (only the reciprocals are kept: smooth_div16)
            lds_f *P = (lds_f *)(W + QG_TILE_BYTES);
            P[2 * lane] = __builtin_amdgcn_rcpf(h2f(hfrom<T>((unsigned short)sm2)));
            P[2 * lane + 1] = __builtin_amdgcn_rcpf(h2f(hfrom<T>((unsigned short)(sm2 >> 16))));
        }
#define QUANT_TAIL_PART 2 // steps 3 and 4: the record read-back, the two groups of the chunk
#include "quantize_tail.inc"
    }

#define QUANT_TAIL_PART 3 // step 5: low rank, the fixed-order combine
#include "quantize_tail.inc"
}

template <int DT, int ACT>
static int launch_quantize_glu(const svdq_quantize_glu_args *a, hipStream_t st) {
    const int KP = a->K / 128, slices = (KP + 3) / 4;
    const int mode = quantize_tail_mode(a->lora_act, a->M_pad, a->R, slices, a->lora_act_format, a->lora_act_zeroed, st);
    GluParams p{a->value, a->gate, a->smooth, a->lora_down, (uint8_t *)a->act, a->ascales, a->lora_act, a->ld_value, a->ld_gate, a->M, a->K, a->R, mode};
    const dim3 grid((unsigned)((size_t)(a->M_pad / 32) * slices)), block(256);
    if (a->smooth) hipLaunchKernelGGL((quantize_glu_kernel<DT, ACT, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((quantize_glu_kernel<DT, ACT, false>), grid, block, 0, st, p);
    return hip_check(hipGetLastError(), "svdq_quantize_glu_halves launch");
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_quantize_glu_halves(const svdq_quantize_glu_args *a, void *stream) {
    if (!a) { set_error("svdq_quantize_glu_halves: args is NULL"); return SVDQ_E_INVALID; }
    if (!a->value || !a->gate || !a->act || !a->ascales) { set_error("svdq_quantize_glu_halves: value, gate, act and ascales are required"); return SVDQ_E_INVALID; }
    if (a->act_fn != SVDQ_GLU_SILU && a->act_fn != SVDQ_GLU_GELU_ERF) { set_error("svdq_quantize_glu_halves: unknown act_fn %d", a->act_fn); return SVDQ_E_INVALID; }
    if (a->lora_act_format != SVDQ_LORA_ACT_F32 && a->lora_act_format != SVDQ_LORA_ACT_Q32 && a->lora_act_format != SVDQ_LORA_ACT_Q32_RUNS) {
        set_error("svdq_quantize_glu_halves: unknown lora_act_format %d", a->lora_act_format);
        return SVDQ_E_INVALID;
    }
    if (a->M <= 0 || a->M_pad < a->M || a->M_pad % 256) {
        set_error("svdq_quantize_glu_halves: need 0 < M=%d <= M_pad=%d and M_pad %% 256 == 0", a->M, a->M_pad);
        return SVDQ_E_INVALID;
    }
    if (a->K <= 0 || a->K % 128) { set_error("svdq_quantize_glu_halves: K=%d must be a positive multiple of 128", a->K); return SVDQ_E_INVALID; }
    if (a->ld_value < a->K || a->ld_value % 8 || a->ld_gate < a->K || a->ld_gate % 8) {
        set_error("svdq_quantize_glu_halves: ld_value=%d and ld_gate=%d must be >= K and multiples of 8", a->ld_value, a->ld_gate);
        return SVDQ_E_INVALID;
    }
    if (a->R < 0 || a->R % 16 || a->R > 256) { set_error("svdq_quantize_glu_halves: R=%d must be a multiple of 16 in [0, 256]", a->R); return SVDQ_E_INVALID; }
    if (a->R > 0 && (!a->lora_down || !a->lora_act)) { set_error("svdq_quantize_glu_halves: R > 0 needs lora_down and lora_act"); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->value | (uintptr_t)a->gate | (uintptr_t)a->act | (uintptr_t)a->lora_down) & 15) {
        set_error("svdq_quantize_glu_halves: value, gate, act and lora_down must be 16-byte aligned");
        return SVDQ_E_INVALID;
    }
    if ((uintptr_t)a->smooth & 3) { set_error("svdq_quantize_glu_halves: smooth must be 4-byte aligned"); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->ascales & 1) || ((uintptr_t)a->lora_act & (a->lora_act_format != SVDQ_LORA_ACT_F32 ? 7 : 3))) {
        set_error("svdq_quantize_glu_halves: ascales must be 2-byte aligned, lora_act 4-byte aligned in fp32 and 8-byte in the Q31.32 formats");
        return SVDQ_E_INVALID;
    }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("svdq_quantize_glu_halves: unknown dtype %d", a->dtype); return SVDQ_E_INVALID; }
    // addressing reach: rows are addressed in 64 bits; the lora_down slab goes through a buffer descriptor with 32-bit byte offsets
    // (ranks R .. R + 31 of the last slab must fall beyond the descriptor's range, not wrap around 2^32)
    if ((long long)a->R * a->K * 2 > 0x7fffffffLL || (a->R > 0 && (long long)(a->R + 32) * a->K * 2 > 0xffffffffLL)) {
        set_error("svdq_quantize_glu_halves: R * K * 2 = %lld bytes of lora_down exceed the 2147483647 the slab loads reach", (long long)a->R * a->K * 2);
        return SVDQ_E_UNSUPPORTED;
    }
    if ((long long)(a->M_pad / 32) * ((a->K / 128 + 3) / 4) > 0x7fffffffLL) {
        set_error("svdq_quantize_glu_halves: M_pad=%d x K=%d needs more than 2147483647 workgroups", a->M_pad, a->K);
        return SVDQ_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    // algorithmic bytes: both halves in, codes + scales + lora_act out, lora_down in (once)
    const double bytes = (double)a->M * a->K * 4 + (double)a->M_pad * a->K * 3 / 4 + (double)a->M_pad * (a->K / 64) * 2 + (double)a->M_pad * a->R * 4 + (double)a->K * a->R * 2;
    const int prof = prof_begin(1, bytes, st);
    int rc;
    if (a->dtype == SVDQ_BF16) rc = a->act_fn == SVDQ_GLU_SILU ? launch_quantize_glu<SVDQ_BF16, SVDQ_GLU_SILU>(a, st) : launch_quantize_glu<SVDQ_BF16, SVDQ_GLU_GELU_ERF>(a, st);
    else rc = a->act_fn == SVDQ_GLU_SILU ? launch_quantize_glu<SVDQ_FP16, SVDQ_GLU_SILU>(a, st) : launch_quantize_glu<SVDQ_FP16, SVDQ_GLU_GELU_ERF>(a, st);
    prof_end(prof, st);
    return rc;
}
