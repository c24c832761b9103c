// The back end the tile quantisers share (quantize_glu.hip, quantize_dwconv_glu.hip): a wave holds one F6 chunk of x -- 32 rows x 128 channels,
// 16-bit -- in its 8 KiB LDS tile, 16-byte pieces XOR-swizzled by the row (piece c16 of row q at q * 256 + ((c16 ^ (q & 15)) << 4)), and 1 / smooth
// of the chunk's channels behind it.  From there on the kernels are one text, quantize_tail.inc: the record read-back, the group quantiser of
// quantize.hip expression for expression, the LDS-DMA of the lora_down slab into the dead tile, the low-rank MFMAs and the fixed-order combine
// of the four waves.  How the tile is produced is the including kernel's own business.
//
// quantize_tail.inc is a fragment of a kernel body, included three times with QUANT_TAIL_PART set (a function the steps were moved into changed
// quantize_glu_kernel's register allocation: 100 bytes of scratch at the same 168 VGPRs; the included text compiles to the instructions it had):
//   1  declarations, ahead of the kernel's own loads: the record xv, the slab offsets, lora_down's descriptor, slab_dma
//   2  steps 3 and 4, inside `if (active)`, behind the tile's last write (with QUANT_TAIL_READBACK_ONLY defined: step 3 alone, for a kernel whose
//      quantiser is its own text -- quantize_mxfp4.hip)
//   3  step 5, outside it: it holds the workgroup's barriers
// It expects in scope: DT, SMOOTH, T, V8, `lds` (the workgroup's 4 * QG_WAVE_BYTES), W (the wave's region), wave, lane, r = lane & 31, h = lane >> 5,
// K, KP, rt (the 32-row tile), kp (the chunk), active, and `p` with lora_down, act, ascales, lora_act, R and mode (lora_act_add's).
#pragma once

#include "glu_act.h" // glu_silu, glu_gelu
#include "svdq_common.h"

namespace svdq {

constexpr int QG_TILE_BYTES = 32 * 256; // the wave's x tile [32 rows][128 channels] 16-bit; later the lora_down slab [32 ranks][128 channels]; later the parked sums
constexpr int QG_RS_BYTES = 128 * 4;    // 1 / smooth of the chunk's channels, fp32, channel order
constexpr int QG_WAVE_BYTES = QG_TILE_BYTES + QG_RS_BYTES;

typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) v4f lds_v4f;
typedef __attribute__((address_space(3))) v4i lds_v4i;
typedef __attribute__((address_space(3))) v2i lds_v2i;
typedef __attribute__((address_space(3))) v16f lds_v16f;
typedef __attribute__((address_space(3))) float lds_f;
typedef __attribute__((address_space(3))) void lds_void;

// clears lora_act ahead of a K-sliced launch (a kernel, not hipMemsetAsync: the launch may be recorded into a graph)
static __global__ __launch_bounds__(256) void quantize_tail_clear(uint32_t *dst, size_t words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) dst[i] = 0u;
}
// the lora_act_add mode of a launch over `slices` K slices, behind the clearing kernel where the slices meet in atomics
static inline int quantize_tail_mode(void *lora_act, int M_pad, int R, int slices, int format, int zeroed, hipStream_t st) {
    const int q32 = format != SVDQ_LORA_ACT_F32;
    if (R > 0 && slices > 1 && !zeroed) {
        const size_t words = (size_t)M_pad * R * (q32 ? 2 : 1);
        const size_t blocks = (words + 1023) / 1024;
        hipLaunchKernelGGL(quantize_tail_clear, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, (uint32_t *)lora_act, words);
    }
    return (slices > 1 ? 1 : 0) | (q32 ? 2 : 0);
}

} // namespace svdq
