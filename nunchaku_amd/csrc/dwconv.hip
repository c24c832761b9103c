// svdq_dwconv3x3: the depthwise 3x3 convolution of SANA's GLU-MBConv (reference: src/kernels/dwconv.cu -- a CUTLASS direct-convolution template
// with a 16-bit accumulator -- called as DWCONV::forward, src/Linear.cpp:542-551, between the two GEMMs of SanaGLUMBConv, src/SanaModel.cpp:192-213).
// Cross-correlation, stride 1, zero padding 1, on a channels-last activation: x and out are [B][H * W, C] token rows (the GEMM's output) with a row
// stride and a batch stride in elements.  Per element, in fp32, in exactly this order:
//
//   acc = bias[c] (or +0);  for ky = 0..2, kx = 0..2:  acc = acc + w[c, ky, kx] * x[h + ky - 1, w + kx - 1, c]   (a tap outside the image: * 0)
//   out[h, w, c] = round16(acc)
//
// A product of two 16-bit values is exact in fp32, so the FMA the adds are written as rounds exactly where a multiply and an add would: only the
// order of the nine additions matters, and it is the one above for every element whatever the schedule (tests/dwconv_ref.py restates it bit for bit).
//
// Schedule.  9 flops per 4 bytes: bound by bytes.  One lane owns 8 channels (one 16-byte piece, as in row_pass.h) and a tile of DW_ROWS x DW_COLS
// output pixels; a wave covers 512 contiguous channels of the tile, so every load and store instruction moves whole 1 KiB lines.  The lane holds
// the nine taps of its channels as fp32 (72 registers, read once from the tap-major [9, C] image) and walks the tile's columns with a sliding
// window of three input columns of DW_ROWS + 2 pixels each, kept as the 16-bit pieces they were loaded as (converted at use: a shift or a
// v_cvt per element, far below the issue rate the byte bound leaves); a fourth column is in flight one step ahead.  An input pixel is therefore
// loaded once per tile: (DW_ROWS + 2) / DW_ROWS x (DW_COLS + 2) / DW_COLS = 1.875 loads per output pixel reach L2, the halo's share is a
// neighbouring tile's own data.  No LDS, no barrier, no atomics, no workspace; one launch.
#include "row_pass.h"

namespace svdq {

constexpr int DW_ROWS = 4;   // output rows of a lane's tile
constexpr int DW_COLS = 8;   // output columns of a lane's tile (the walk)
constexpr int DW_WIN = DW_ROWS + 2;

struct DwParams {
    const uint16_t *x, *taps, *bias;
    uint16_t *out;
    long long x_bs, o_bs; // batch strides in elements
    int ldx, ldo;         // row (token) strides in elements
    int H, W, C;
    int ncb, tiles_w;     // channel blocks of 512, tiles per image row
};

template <typename T> __device__ __forceinline__ f32x2_t dw_pair(int dword) {
    return f32x2_t{h2f(hfrom<T>((unsigned short)((unsigned)dword & 0xffffu))), h2f(hfrom<T>((unsigned short)((unsigned)dword >> 16)))};
}

// one input column of the window: the pixels (h0 - 1 .. h0 + DW_ROWS, w) of the lane's 8 channels; outside the image: zeros, nothing is read
__device__ __forceinline__ void dw_load_column(v4i (&col)[DW_WIN], const uint16_t *xb, int h0, int w, const DwParams &p) {
#pragma unroll
    for (int i = 0; i < DW_WIN; i++) {
        const int h = h0 - 1 + i;
        v4i v = {0, 0, 0, 0};
        if (w >= 0 && w < p.W && h >= 0 && h < p.H) v = *reinterpret_cast<const v4i *>(xb + ((long long)h * p.W + w) * p.ldx);
        col[i] = v;
    }
}

template <int DT>
__global__ __launch_bounds__(64) void dwconv3x3_kernel(const DwParams p) {
    using T = typename Half<DT>::T;
    const unsigned bid = blockIdx.x;
    const int cb = (int)(bid % (unsigned)p.ncb);
    const unsigned tile = bid / (unsigned)p.ncb;
    const int tw = (int)(tile % (unsigned)p.tiles_w), th = (int)(tile / (unsigned)p.tiles_w);
    const int c = (cb * 64 + (int)threadIdx.x) * 8;
    if (c >= p.C) return; // the ragged tail of the last channel block (no barrier below)
    const int h0 = th * DW_ROWS, w0 = tw * DW_COLS;
    const int wend = w0 + DW_COLS < p.W ? w0 + DW_COLS : p.W;

    f32x2_t wt[9][4], b0[4];
#pragma unroll
    for (int t = 0; t < 9; t++) {
        const v4i raw = *reinterpret_cast<const v4i *>(p.taps + (size_t)t * p.C + c);
#pragma unroll
        for (int d = 0; d < 4; d++) wt[t][d] = dw_pair<T>(raw[d]);
    }
    {
        v4i raw = {0, 0, 0, 0}; // (+0 in either format)
        if (p.bias) raw = *reinterpret_cast<const v4i *>(p.bias + c);
#pragma unroll
        for (int d = 0; d < 4; d++) b0[d] = dw_pair<T>(raw[d]);
    }

    const uint16_t *xb = p.x + (long long)blockIdx.y * p.x_bs + c;
    uint16_t *ob = p.out + (long long)blockIdx.y * p.o_bs + c;

    v4i win[3][DW_WIN], ahead[DW_WIN]; // columns w - 1, w, w + 1 and the one in flight
    dw_load_column(win[0], xb, h0, w0 - 1, p);
    dw_load_column(win[1], xb, h0, w0, p);
    dw_load_column(ahead, xb, h0, w0 + 1, p);
    for (int w = w0; w < wend; w++) {
#pragma unroll
        for (int i = 0; i < DW_WIN; i++) win[2][i] = ahead[i];
        if (w + 1 < wend) dw_load_column(ahead, xb, h0, w + 2, p);
#pragma unroll
        for (int r = 0; r < DW_ROWS; r++) {
            if (h0 + r >= p.H) break;
            f32x2_t acc[4] = {b0[0], b0[1], b0[2], b0[3]};
#pragma unroll
            for (int ky = 0; ky < 3; ky++)
#pragma unroll
                for (int kx = 0; kx < 3; kx++)
#pragma unroll
                    for (int d = 0; d < 4; d++)
                        acc[d] = __builtin_elementwise_fma(wt[ky * 3 + kx][d], dw_pair<T>(win[kx][r + ky][d]), acc[d]);
            v4i o;
#pragma unroll
            for (int d = 0; d < 4; d++) o[d] = (int)((unsigned)hbits(f2h<T>(acc[d][0])) | ((unsigned)hbits(f2h<T>(acc[d][1])) << 16));
            *reinterpret_cast<v4i *>(ob + ((long long)(h0 + r) * p.W + w) * p.ldo) = o;
        }
#pragma unroll
        for (int i = 0; i < DW_WIN; i++) { win[0][i] = win[1][i]; win[1][i] = win[2][i]; }
    }
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_dwconv3x3(const svdq_dwconv3x3_args *a, void *stream) {
    const char *op = "svdq_dwconv3x3";
    if (!a) { set_error("%s: args is NULL", op); return SVDQ_E_INVALID; }
    if (!a->x || !a->weight || !a->out) { set_error("%s: x, weight and out are required", op); return SVDQ_E_INVALID; }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("%s: unknown dtype %d", op, a->dtype); return SVDQ_E_INVALID; }
    if (a->B < 1 || a->H < 1 || a->W < 1 || a->C < 1) {
        set_error("%s: need B=%d, H=%d, W=%d, C=%d >= 1", op, a->B, a->H, a->W, a->C);
        return SVDQ_E_INVALID;
    }
    if (a->C % 8) { set_error("%s: C=%d must be a multiple of 8", op, a->C); return SVDQ_E_INVALID; }
    if (a->ldx < a->C || a->ldo < a->C || a->ldx % 8 || a->ldo % 8) {
        set_error("%s: row strides (ldx=%d ldo=%d) must be at least C=%d and a multiple of 8", op, a->ldx, a->ldo, a->C);
        return SVDQ_E_INVALID;
    }
    const long long T = (long long)a->H * a->W;
    if (a->B > 1 && (a->x_bs < T * a->ldx || a->out_bs < T * a->ldo || a->x_bs % 8 || a->out_bs % 8)) {
        set_error("%s: batch strides (x_bs=%lld out_bs=%lld) must be at least H * W * row stride and a multiple of 8", op, (long long)a->x_bs,
                  (long long)a->out_bs);
        return SVDQ_E_INVALID;
    }
    if (!aligned_to(16, {a->x, a->weight, a->bias, a->out})) {
        set_error("%s: x, weight, bias and out must be 16-byte aligned", op);
        return SVDQ_E_INVALID;
    }
    const long long ncb = (a->C + 511) / 512, tiles_w = (a->W + DW_COLS - 1) / DW_COLS, tiles_h = (a->H + DW_ROWS - 1) / DW_ROWS;
    if (a->B > 65535 || ncb * tiles_w * tiles_h > 0x7fffffffLL) {
        set_error("%s: B=%d (at most 65535) or ceil(C/512) * ceil(W/%d) * ceil(H/%d) = %lld (at most 2^31 - 1) exceeds the grid", op, a->B, DW_COLS,
                  DW_ROWS, ncb * tiles_w * tiles_h);
        return SVDQ_E_INVALID;
    }
    // the element spans of the two tensors (all offsets are formed in 64 bits on the device); in place is not supported: a pixel is read by its
    // neighbours' lanes after its own lane has written it
    const long long bx = a->B > 1 ? a->x_bs : 0, bo = a->B > 1 ? a->out_bs : 0;
    const long long xspan = (a->B - 1) * bx + (T - 1) * a->ldx + a->C, ospan = (a->B - 1) * bo + (T - 1) * a->ldo + a->C;
    const uintptr_t x0 = (uintptr_t)a->x, o0 = (uintptr_t)a->out;
    if (x0 < o0 + 2 * (uintptr_t)ospan && o0 < x0 + 2 * (uintptr_t)xspan) {
        set_error("%s: x and out overlap (in place is not supported)", op);
        return SVDQ_E_INVALID;
    }
    DwParams p;
    p.x = (const uint16_t *)a->x; p.taps = (const uint16_t *)a->weight; p.bias = (const uint16_t *)a->bias; p.out = (uint16_t *)a->out;
    p.x_bs = bx; p.o_bs = bo; p.ldx = a->ldx; p.ldo = a->ldo;
    p.H = a->H; p.W = a->W; p.C = a->C; p.ncb = (int)ncb; p.tiles_w = (int)tiles_w;
    const dim3 grid((unsigned)(ncb * tiles_w * tiles_h), a->B);
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == SVDQ_BF16) hipLaunchKernelGGL((dwconv3x3_kernel<SVDQ_BF16>), grid, dim3(64), 0, st, p);
    else hipLaunchKernelGGL((dwconv3x3_kernel<SVDQ_FP16>), grid, dim3(64), 0, st, p);
    return hip_check(hipGetLastError(), "svdq_dwconv3x3 launch");
}
