// svdq_quantize_mxfp4: the MXFP4 activation quantiser.
//
//   v = smooth_div16(x, smooth)                           the rounding point of the INT4 quantiser's smoothing division
//   per (row, 32 channels): amax, X = floor(log2 amax) - 2, scale byte = clamp(X + 127, 0, 254), code = RNE_e2m1(v * 2^-(byte - 127)), saturated to +-6
//   lora_act = x @ lora_down on the un-smoothed x (fp32)
//
// Outputs: the codes as natural rows [M_pad][K / 2] (two e2m1 codes a byte, even channel in the low nibble -- what a lane of
// v_mfma_scale_f32_32x32x64_f8f6f4 reads as one 16-byte block), and the E8M0 bytes packed four K-blocks to a dword, [K / 128][M_pad] dwords
// (byte b of dword (kp, row) = block 4 kp + b): the GEMM's per-K-step scale operand, selected by op_sel.
//
// The tile handling is the tile quantisers' shared back end (quantize_tail.h): a wave owns 32 rows x 128 channels in a swizzled 8 KiB LDS tile, read
// back in record layout; the lora_down slab lands in the dead tile by LDS-DMA, the low-rank MFMAs and the fixed-order combine of the four waves
// are quantize_tail.inc parts 1 and 3.  The block quantiser between them is mxfp4_block.h, which the GEMM's GELU_QUANT epilogue shares.
#include "mxfp4_block.h"
#include "quantize_tail.h"

namespace svdq {

struct Mxfp4QuantParams {
    const void *x, *smooth, *lora_down;
    uint8_t *act;
    uint32_t *ascales;
    void *lora_act;
    long long ldx;
    int M, M_pad, K, R, mode;
};

template <int DT, bool SMOOTH>
__global__ __launch_bounds__(256, 3) void quantize_mxfp4_kernel(Mxfp4QuantParams p) {
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
    lds_u8 *const W = (lds_u8 *)lds + wave * QG_WAVE_BYTES;

#define QUANT_TAIL_PART 1 // the record, the slab offsets, slab_dma
#include "quantize_tail.inc"

    if (active) {
        // ---- 1. the chunk's loads, row-contiguous: lane (rr, c16) takes 16 bytes of rows 4i + rr.  A row >= M reads the last row and is zeroed below
        const int c16 = lane & 15, rr = lane >> 4;
        v4i xl[8];
        bool live[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int row = rt * 32 + 4 * i + rr;
            live[i] = row < p.M;
            xl[i] = *reinterpret_cast<const v4i *>((const T *)p.x + (size_t)(live[i] ? row : p.M - 1) * p.ldx + kp * 128 + 8 * c16);
        }
        unsigned sm2 = 0;
        if constexpr (SMOOTH) sm2 = *reinterpret_cast<const unsigned *>((const T *)p.smooth + kp * 128 + 2 * lane);
        // ---- 2. -> LDS tile, piece c16 of row q at q * 256 + ((c16 ^ (q & 15)) << 4)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int q = 4 * i + rr;
            *(lds_v4i *)(W + q * 256 + ((c16 ^ (q & 15)) << 4)) = live[i] ? xl[i] : v4i{0, 0, 0, 0};
        }
        if constexpr (SMOOTH) {
            lds_f *P = (lds_f *)(W + QG_TILE_BYTES);
            P[2 * lane] = __builtin_amdgcn_rcpf(h2f(hfrom<T>((unsigned short)sm2)));
            P[2 * lane + 1] = __builtin_amdgcn_rcpf(h2f(hfrom<T>((unsigned short)(sm2 >> 16))));
        }
#define QUANT_TAIL_READBACK_ONLY // step 3: back in record layout (row r, channels 64 grp + 8 tc + 4 h + e); the dead tile takes the first lora_down slab
#define QUANT_TAIL_PART 2
#include "quantize_tail.inc"
#undef QUANT_TAIL_READBACK_ONLY

        // ---- 4. the chunk's four 32-channel blocks.  Of block b the lane holds pieces q = 0 .. 3: channels 32 b + 8 q + 4 h + e, 4 codes = 16 bits
        unsigned pc[4][2], sdw = 0; // pc[b][t] = piece 2t | piece 2t + 1 << 16
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int grp = b >> 1;
            float v[16], amax = 0.f;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int tc = 4 * (b & 1) + q;
                v4f rs = {};
                if constexpr (SMOOTH) rs = *(const lds_v4f *)(W + QG_TILE_BYTES + (grp * 64 + 8 * tc + 4 * h) * 4);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float xf = h2f(hfrom<T>((unsigned short)((unsigned)xv[grp][tc][e >> 1] >> (16 * (e & 1)))));
                    if constexpr (SMOOTH) xf = smooth_div16<T>(xf, rs[e]);
                    v[4 * q + e] = xf;
                    amax = mx_amax_acc(amax, xf);
                }
            }
            const unsigned sb = mx_block_byte<T>(amax);
            MX_BLOCK_CODES(v, sb, pc[b]);
            sdw |= sb << (8 * b);
        }
        unsigned dw[8];
        mx_trade_halves(pc, h, dw);
        uint8_t *dst = p.act + (size_t)(rt * 32 + r) * (K / 2) + kp * 64 + 32 * h;
        *reinterpret_cast<uint4 *>(dst) = make_uint4(dw[0], dw[1], dw[2], dw[3]);
        *reinterpret_cast<uint4 *>(dst + 16) = make_uint4(dw[4], dw[5], dw[6], dw[7]);
        if (h == 0) p.ascales[(size_t)kp * p.M_pad + rt * 32 + r] = sdw;
    }

#define QUANT_TAIL_PART 3 // low rank, the fixed-order combine
#include "quantize_tail.inc"
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_quantize_mxfp4(const svdq_quantize_mxfp4_args *a, void *stream) {
    if (!a) { set_error("svdq_quantize_mxfp4: args is NULL"); return SVDQ_E_INVALID; }
    if (!a->x || !a->act || !a->ascales) { set_error("svdq_quantize_mxfp4: x, act and ascales are required"); return SVDQ_E_INVALID; }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("svdq_quantize_mxfp4: unknown dtype %d", a->dtype); return SVDQ_E_INVALID; }
    if (a->M <= 0 || a->M_pad < a->M || a->M_pad % 256) {
        set_error("svdq_quantize_mxfp4: need 0 < M=%d <= M_pad=%d and M_pad %% 256 == 0", a->M, a->M_pad);
        return SVDQ_E_INVALID;
    }
    if (a->K <= 0 || a->K % 128) { set_error("svdq_quantize_mxfp4: K=%d must be a positive multiple of 128", a->K); return SVDQ_E_INVALID; }
    if (a->ldx < a->K || a->ldx % 8) { set_error("svdq_quantize_mxfp4: ldx=%d must be >= K and a multiple of 8", a->ldx); return SVDQ_E_INVALID; }
    if (a->R < 0 || a->R % 16 || a->R > 256) { set_error("svdq_quantize_mxfp4: R=%d must be a multiple of 16 in [0, 256]", a->R); return SVDQ_E_INVALID; }
    if (a->R > 0 && (!a->lora_down || !a->lora_act)) { set_error("svdq_quantize_mxfp4: R > 0 needs lora_down and lora_act"); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->x | (uintptr_t)a->act | (uintptr_t)a->lora_down) & 15) {
        set_error("svdq_quantize_mxfp4: x, act and lora_down must be 16-byte aligned");
        return SVDQ_E_INVALID;
    }
    if (((uintptr_t)a->smooth | (uintptr_t)a->ascales | (uintptr_t)a->lora_act) & 3) {
        set_error("svdq_quantize_mxfp4: smooth, ascales and lora_act must be 4-byte aligned");
        return SVDQ_E_INVALID;
    }
    // addressing reach: rows are addressed in 64 bits; the lora_down slab goes through a buffer descriptor with 32-bit byte offsets
    if ((long long)a->R * a->K * 2 > 0x7fffffffLL || (a->R > 0 && (long long)(a->R + 32) * a->K * 2 > 0xffffffffLL)) {
        set_error("svdq_quantize_mxfp4: R * K * 2 = %lld bytes of lora_down exceed the 2147483647 the slab loads reach", (long long)a->R * a->K * 2);
        return SVDQ_E_UNSUPPORTED;
    }
    const int KP = a->K / 128, slices = (KP + 3) / 4;
    if ((long long)(a->M_pad / 32) * slices > 0x7fffffffLL) {
        set_error("svdq_quantize_mxfp4: M_pad=%d x K=%d needs more than 2147483647 workgroups", a->M_pad, a->K);
        return SVDQ_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    const double bytes = (double)a->M * a->K * 2 + (double)a->M_pad * a->K / 2 + (double)a->M_pad * (a->K / 32) + (double)a->M_pad * a->R * 4 + (double)a->K * a->R * 2;
    const int prof = prof_begin(1, bytes, st);
    const int mode = quantize_tail_mode(a->lora_act, a->M_pad, a->R, slices, SVDQ_LORA_ACT_F32, a->lora_act_zeroed, st);
    Mxfp4QuantParams p{a->x, a->smooth, a->lora_down, (uint8_t *)a->act, (uint32_t *)a->ascales, a->lora_act, a->ldx, a->M, a->M_pad, a->K, a->R, mode};
    const dim3 grid((unsigned)((size_t)(a->M_pad / 32) * slices)), block(256);
    if (a->dtype == SVDQ_BF16) {
        if (a->smooth) hipLaunchKernelGGL((quantize_mxfp4_kernel<SVDQ_BF16, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((quantize_mxfp4_kernel<SVDQ_BF16, false>), grid, block, 0, st, p);
    } else {
        if (a->smooth) hipLaunchKernelGGL((quantize_mxfp4_kernel<SVDQ_FP16, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((quantize_mxfp4_kernel<SVDQ_FP16, false>), grid, block, 0, st, p);
    }
    const int rc = hip_check(hipGetLastError(), "svdq_quantize_mxfp4 launch");
    prof_end(prof, st);
    return rc;
}
