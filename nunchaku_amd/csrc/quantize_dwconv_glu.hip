// svdq_quantize_dwconv_glu: SANA's depthwise 3x3 convolution (dwconv.hip), the interleaved GLU of quantize.hip's fuse_glu and the W4A4 activation
// quantiser in one launch.  y is [B][H * W, C] token rows (the first GEMM's output), taps the tap-major [9, C] image, row m = b H W + h W + w:
//
//   c[m, ch] = round16(fp32: acc = bias[ch] (or +0); for ky, kx row-major: acc = fma(w[ch, ky, kx], y[b, h + ky - 1, w + kx - 1, ch], acc))
//                                                         -- dwconv.hip's arithmetic and order; a tap outside the image multiplies a zero
//   a = round16(silu(c[m, 2k + 1])),  x[m, k] = round16(c[m, 2k] * a)          -- glu_silu, the 16-bit multiply; conv channels >= C are zero
//   then everything svdq_quantize_w4a4_act_fuse_lora does to x [M = B H W, K]
// so the 16-bit [M, 2K] convolution output never exists in HBM.
//
// Design.  The unit of work is quantize_glu_kernel's: a wave owns one F6 chunk, 32 consecutive rows x 128 quantised channels
// = 256 conv channels, a workgroup four neighbouring chunks of one row tile, and from the LDS tile on the kernels are one text (quantize_tail.inc).
// What is new is how the chunk comes in:
//   * lane (pc, hh) owns piece pc of the chunk -- 8 conv channels, 16 bytes, 4 (value, gate) pairs -- for rows 16 hh .. 16 hh + 15: 32 lanes read
//     512 contiguous bytes of one pixel.  It holds its nine taps and the bias as fp32 (80 registers) and walks its 16 tokens with a sliding window
//     of three columns x three grid rows kept as the 16-byte pieces they were loaded as; the column one step ahead is in flight while the current
//     pixel is computed.  Rows are consecutive tokens: where the walk leaves a grid row (or a sample) the window is loaded afresh; rows h - 1 and
//     h + 1 are taken from the lane's own sample or are zeros, nothing is read there;
//   * per pixel the lane rounds its 8 conv outputs, applies the GLU to the four pairs and writes 8 bytes of x into the wave's swizzled tile.
// Halo: a 16-token walk inside one grid row loads 3 x 18 pieces for 16 outputs, 3.4 per output piece (3.2 for the wave's 32 rows: the two halves'
// shared columns hit L1).  The reuse is left to L2, and the workgroup order is made for it: a workgroup's index is first mapped to the XCD it was
// dispatched to (index mod 8), every XCD gets one contiguous run of the (K slice, row tile) order, slice-major -- so the workgroups that read the
// grid rows above and below a strip run on the same XCD, W / 32 workgroups apart, and find them in its L2.
#include "quantize_tail.h"

namespace svdq {

constexpr int DG_XCDS = 8; // workgroups are dispatched round-robin over the chip's XCDs, each with an L2 of its own

struct DwGluParams {
    const uint16_t *y, *taps, *bias;
    const void *smooth, *lora_down;
    uint8_t *act;
    void *ascales, *lora_act;
    long long y_bs; // batch stride in elements
    int ldy;        // row (token) stride in elements
    int H, W, C;
    int M, K, R, mode; // mode: lora_act_add's (bit 0 = K is sliced over workgroups, bit 1 = Q31.32)
    int row_tiles;     // M_pad / 32
};

// one column of the window: the lane's piece of the pixels (h - 1 .. h + 1, w); a row or column outside the image: zeros, nothing is read
__device__ __forceinline__ void dg_load_column(v4i (&col)[3], const uint16_t *(&rowp)[3], int w, const DwGluParams &p) {
#pragma unroll
    for (int ky = 0; ky < 3; ky++) {
        v4i v = {0, 0, 0, 0};
        if (rowp[ky] != nullptr && w >= 0 && w < p.W) v = *reinterpret_cast<const v4i *>(rowp[ky] + (long long)w * p.ldy);
        col[ky] = v;
    }
}

template <int DT, bool SMOOTH>
__global__ __launch_bounds__(256, 3) void quantize_dwconv_glu_kernel(DwGluParams p) {
    using T = typename Half<DT>::T;
    using V8 = typename Half<DT>::V8;
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * QG_WAVE_BYTES];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int r = lane & 31, h = lane >> 5;
    const int K = p.K, KP = K / 128;
    // the XCD-aware order: XCD x runs workgroups x, x + 8, ...; it gets the logical indices [x per + min(x, rem), ...), slice-major
    const unsigned per = gridDim.x / DG_XCDS, rem = gridDim.x % DG_XCDS, xcd = blockIdx.x % DG_XCDS;
    const unsigned logical = xcd * per + (xcd < rem ? xcd : rem) + blockIdx.x / DG_XCDS;
    const int rt = (int)(logical % (unsigned)p.row_tiles), kp = (int)(logical / (unsigned)p.row_tiles) * 4 + wave;
    const bool active = kp < KP; // wave-uniform
    lds_u8 *const W = (lds_u8 *)lds + wave * QG_WAVE_BYTES; // private to the wave until the combine

#define QUANT_TAIL_PART 1 // the record, the slab offsets, slab_dma
#include "quantize_tail.inc"

    if (active) {
        // ---- 1. the lane's taps and bias, fp32 (a piece of absent conv channels, c >= C, is zeros: 0 * silu(0) = 0)
        const int pc = lane & 31, hh = lane >> 5;
        const int c = kp * 256 + pc * 8;
        const bool have = c < p.C;
        float wt[9][8], b0[8];
#pragma unroll
        for (int t = 0; t < 9; t++) {
            v4i raw = {0, 0, 0, 0};
            if (have) raw = *reinterpret_cast<const v4i *>(p.taps + (size_t)t * p.C + c);
#pragma unroll
            for (int e = 0; e < 8; e++) wt[t][e] = h2f(hfrom<T>((unsigned short)((unsigned)raw[e >> 1] >> (16 * (e & 1)))));
        }
        {
            v4i raw = {0, 0, 0, 0}; // (+0 in either format)
            if (have && p.bias) raw = *reinterpret_cast<const v4i *>(p.bias + c);
#pragma unroll
            for (int e = 0; e < 8; e++) b0[e] = h2f(hfrom<T>((unsigned short)((unsigned)raw[e >> 1] >> (16 * (e & 1)))));
        }
        unsigned sm2 = 0;
        if constexpr (SMOOTH) sm2 = *reinterpret_cast<const unsigned *>((const T *)p.smooth + kp * 128 + 2 * lane);

        // ---- 2. the walk over rows m0 .. m0 + 15: (b, hy, wx) of the current row, the window [kx][ky] around it
        int m = rt * 32 + 16 * hh;
        const int HW = p.H * p.W;
        int b = m / HW, hy = (m - b * HW) / p.W, wx = m - b * HW - hy * p.W;
        const uint16_t *rowp[3] = {nullptr, nullptr, nullptr}; // grid rows hy - 1, hy, hy + 1 of sample b at the lane's channels; nullptr: outside
        v4i win[3][3], ahead[3];
        bool fresh = true;
#pragma unroll 1
        for (int i = 0; i < 16; i++, m++) {
            v2i xo = {0, 0};
            if (have && m < p.M) { // (a row >= M: zeros, as the padding rows of every quantiser)
                if (fresh) {
                    const uint16_t *yb = p.y + (long long)b * p.y_bs + c;
#pragma unroll
                    for (int ky = 0; ky < 3; ky++) {
                        const int hr = hy - 1 + ky;
                        rowp[ky] = hr >= 0 && hr < p.H ? yb + (long long)hr * p.W * p.ldy : nullptr;
                    }
                    dg_load_column(win[0], rowp, wx - 1, p);
                    dg_load_column(win[1], rowp, wx, p);
                    dg_load_column(ahead, rowp, wx + 1, p);
                }
#pragma unroll
                for (int ky = 0; ky < 3; ky++) win[2][ky] = ahead[ky];
                if (wx + 1 < p.W && i + 1 < 16) dg_load_column(ahead, rowp, wx + 2, p); // (the next pixel of this walk needs it)
                float acc[8];
#pragma unroll
                for (int e = 0; e < 8; e++) acc[e] = b0[e];
#pragma unroll
                for (int ky = 0; ky < 3; ky++)
#pragma unroll
                    for (int kx = 0; kx < 3; kx++)
#pragma unroll
                        for (int e = 0; e < 8; e++) {
                            const float yv = h2f(hfrom<T>((unsigned short)((unsigned)win[kx][ky][e >> 1] >> (16 * (e & 1)))));
                            acc[e] = __builtin_fmaf(wt[ky * 3 + kx][e], yv, acc[e]);
                        }
                // the interleaved GLU on the rounded conv outputs: value = channel 2k, gate = channel 2k + 1
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float v = round16<T>(acc[2 * k]), g = round16<T>(acc[2 * k + 1]);
                    const float a = round16<T>(glu_silu(g));
                    xo[k >> 1] |= (int)((unsigned)hbits(f2h<T>(v * a)) << (16 * (k & 1)));
                }
#pragma unroll
                for (int ky = 0; ky < 3; ky++) { win[0][ky] = win[1][ky]; win[1][ky] = win[2][ky]; }
            }
            // x in the walk's layout -> LDS tile: the lane's 8 bytes are half pc & 1 of piece pc >> 1 of row q
            const int q = 16 * hh + i;
            *(lds_v2i *)(W + q * 256 + (((pc >> 1) ^ (q & 15)) << 4) + 8 * (pc & 1)) = xo;
            fresh = false;
            if (++wx == p.W) { // the walk leaves the grid row, and with the last one the sample
                wx = 0; fresh = true;
                if (++hy == p.H) { hy = 0; b++; }
            }
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

template <int DT>
static int launch_quantize_dwconv_glu(const svdq_quantize_dwconv_glu_args *a, hipStream_t st) {
    const int KP = a->K / 128, slices = (KP + 3) / 4;
    const int mode = quantize_tail_mode(a->lora_act, a->M_pad, a->R, slices, a->lora_act_format, a->lora_act_zeroed, st);
    DwGluParams p{(const uint16_t *)a->x, (const uint16_t *)a->weight, (const uint16_t *)a->bias, a->smooth, a->lora_down, (uint8_t *)a->act, a->ascales,
                  a->lora_act, a->B > 1 ? (long long)a->x_bs : 0, a->ldx, a->H, a->W, a->C, a->B * a->H * a->W, a->K, a->R, mode, a->M_pad / 32};
    const dim3 grid((unsigned)((size_t)(a->M_pad / 32) * slices)), block(256);
    if (a->smooth) hipLaunchKernelGGL((quantize_dwconv_glu_kernel<DT, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((quantize_dwconv_glu_kernel<DT, false>), grid, block, 0, st, p);
    return hip_check(hipGetLastError(), "svdq_quantize_dwconv_glu launch");
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_quantize_dwconv_glu(const svdq_quantize_dwconv_glu_args *a, void *stream) {
    const char *op = "svdq_quantize_dwconv_glu";
    if (!a) { set_error("%s: args is NULL", op); return SVDQ_E_INVALID; }
    if (!a->x || !a->weight || !a->act || !a->ascales) { set_error("%s: x, weight, act and ascales are required", op); return SVDQ_E_INVALID; }
    if (a->lora_act_format != SVDQ_LORA_ACT_F32 && a->lora_act_format != SVDQ_LORA_ACT_Q32 && a->lora_act_format != SVDQ_LORA_ACT_Q32_RUNS) {
        set_error("%s: unknown lora_act_format %d", op, a->lora_act_format);
        return SVDQ_E_INVALID;
    }
    if (a->B < 1 || a->H < 1 || a->W < 1 || a->C < 1) { set_error("%s: need B=%d, H=%d, W=%d, C=%d >= 1", op, a->B, a->H, a->W, a->C); return SVDQ_E_INVALID; }
    const long long tokens = (long long)a->H * a->W, M = tokens * a->B;
    if (M > a->M_pad || a->M_pad % 256) {
        set_error("%s: need B * H * W = %lld <= M_pad=%d and M_pad %% 256 == 0", op, M, a->M_pad);
        return SVDQ_E_INVALID;
    }
    if (a->K <= 0 || a->K % 128) { set_error("%s: K=%d must be a positive multiple of 128", op, a->K); return SVDQ_E_INVALID; }
    if (a->C % 8 || a->C > 2 * (long long)a->K) { set_error("%s: C=%d must be a multiple of 8, at most 2K = %lld", op, a->C, 2 * (long long)a->K); return SVDQ_E_INVALID; }
    if (a->ldx < a->C || a->ldx % 8) { set_error("%s: the row stride ldx=%d must be >= C=%d and a multiple of 8", op, a->ldx, a->C); return SVDQ_E_INVALID; }
    if (a->B > 1 && (a->x_bs < tokens * a->ldx || a->x_bs % 8)) {
        set_error("%s: the batch stride x_bs=%lld must be at least H * W * ldx = %lld and a multiple of 8", op, (long long)a->x_bs, tokens * a->ldx);
        return SVDQ_E_INVALID;
    }
    if (a->R < 0 || a->R % 16 || a->R > 256) { set_error("%s: R=%d must be a multiple of 16 in [0, 256]", op, a->R); return SVDQ_E_INVALID; }
    if (a->R > 0 && (!a->lora_down || !a->lora_act)) { set_error("%s: R > 0 needs lora_down and lora_act", op); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->x | (uintptr_t)a->weight | (uintptr_t)a->bias | (uintptr_t)a->act | (uintptr_t)a->lora_down) & 15) {
        set_error("%s: x, weight, bias, act and lora_down must be 16-byte aligned", op);
        return SVDQ_E_INVALID;
    }
    if ((uintptr_t)a->smooth & 3) { set_error("%s: smooth must be 4-byte aligned", op); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->ascales & 1) || ((uintptr_t)a->lora_act & (a->lora_act_format != SVDQ_LORA_ACT_F32 ? 7 : 3))) {
        set_error("%s: ascales must be 2-byte aligned, lora_act 4-byte aligned in fp32 and 8-byte in the Q31.32 formats", op);
        return SVDQ_E_INVALID;
    }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("%s: unknown dtype %d", op, a->dtype); return SVDQ_E_INVALID; }
    // addressing reach: pixels are addressed in 64 bits; the lora_down slab goes through a buffer descriptor with 32-bit byte offsets
    // (ranks R .. R + 31 of the last slab must fall beyond the descriptor's range, not wrap around 2^32)
    if ((long long)a->R * a->K * 2 > 0x7fffffffLL || (a->R > 0 && (long long)(a->R + 32) * a->K * 2 > 0xffffffffLL)) {
        set_error("%s: R * K * 2 = %lld bytes of lora_down exceed the 2147483647 the slab loads reach", op, (long long)a->R * a->K * 2);
        return SVDQ_E_UNSUPPORTED;
    }
    if ((long long)(a->M_pad / 32) * ((a->K / 128 + 3) / 4) > 0x7fffffffLL) {
        set_error("%s: M_pad=%d x K=%d needs more than 2147483647 workgroups", op, a->M_pad, a->K);
        return SVDQ_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    // algorithmic bytes: y and the taps in, codes + scales + lora_act out, lora_down in (once)
    const double bytes = (double)M * a->C * 2 + (double)a->C * 20 + (double)a->M_pad * a->K * 3 / 4 + (double)a->M_pad * (a->K / 64) * 2 +
                         (double)a->M_pad * a->R * 4 + (double)a->K * a->R * 2;
    const int prof = prof_begin(1, bytes, st);
    const int rc = a->dtype == SVDQ_BF16 ? launch_quantize_dwconv_glu<SVDQ_BF16>(a, st) : launch_quantize_dwconv_glu<SVDQ_FP16>(a, st);
    prof_end(prof, st);
    return rc;
}
