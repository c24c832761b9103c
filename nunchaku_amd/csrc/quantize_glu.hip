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
#include "svdq_common.h"

namespace svdq {

constexpr int QG_TILE_BYTES = 32 * 256; // the wave's x tile [32 rows][128 channels] 16-bit; later the lora_down slab [32 ranks][128 channels]; later the parked sums
constexpr int QG_RS_BYTES = 128 * 4;    // 1 / smooth of the chunk's channels, fp32, channel order
constexpr int QG_WAVE_BYTES = QG_TILE_BYTES + QG_RS_BYTES;

struct GluParams {
    const void *value, *gate, *smooth, *lora_down;
    uint8_t *act;
    void *ascales, *lora_act;
    long long ld_value, ld_gate;
    int M, K, R, mode; // mode: lora_act_add's (bit 0 = K is sliced over workgroups, bit 1 = Q31.32)
};

// silu(g) = g * rcp(1 + exp2(-log2e g)): the form of quantize_kernel's GLU front end, bit for bit, down to g = -44.  Below, 1 + e == e in fp32 and e
// itself leaves the range at g = -88.7 although g e^g is an ordinary bf16 number down to g = -96: the exponent is carried 2^64 lower and put back
// with a multiply, which rounds into the fp32 subnormals where v_rcp_f32 would flush.
__device__ __forceinline__ float glu_silu(float g) {
    const bool big = g < -44.0f;
    const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * g - (big ? 64.0f : 0.0f));
    const float sg = g * __builtin_amdgcn_rcpf(big ? e : 1.0f + e);
    return big ? sg * 0x1p-64f : sg;
}
// gelu(g) = g * 0.5 * (1 + erf(g sqrt(1/2))) with 1 + erf(z) taken as erfc(|z|) or 2 - erfc(|z|): the same function (within 2^-23 of the
// literal form where that form is accurate), and accurate in the negative tail, where 1 + erf cancels (gelu(-6) = -6e-9 is an ordinary 16-bit number).
__device__ __forceinline__ float glu_gelu(float g) {
    const float z = g * 0.70710678118654752440f;
    const float c = erfcf(__builtin_fabsf(z));
    return g * (0.5f * (z < 0.f ? c : 2.0f - c));
}

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
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
    typedef __attribute__((address_space(3))) v4f lds_v4f;
    typedef __attribute__((address_space(3))) v4i lds_v4i;
    typedef __attribute__((address_space(3))) v2i lds_v2i;
    typedef __attribute__((address_space(3))) v16f lds_v16f;
    typedef __attribute__((address_space(3))) float lds_f;
    typedef __attribute__((address_space(3))) void lds_void;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int r = lane & 31, h = lane >> 5;
    const int K = p.K, KP = K / 128;
    const int slices = (KP + 3) / 4;
    const int rt = blockIdx.x / slices, kp = (blockIdx.x % slices) * 4 + wave;
    const bool active = kp < KP; // wave-uniform
    lds_u8 *const W = (lds_u8 *)lds + wave * QG_WAVE_BYTES; // private to the wave until the combine

    v2i xv[2][8]; // the lane's record: row r, channels 64 grp + 8 tc + 4 h + e
#pragma unroll
    for (int i = 0; i < 16; i++) xv[i >> 3][i & 7] = v2i{0, 0};
    unsigned ldo[4] = {0, 0, 0, 0}; // lora_down slab offsets of DMA instructions i = j, j + 4 (rank 4j + lane / 16 [+ 16]; the swizzle only depends on j)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned rank = 4 * j + (lane >> 4);
        ldo[j] = (rank * (unsigned)K + kp * 128 + (((lane & 15) ^ (rank & 15)) * 8)) * 2u;
    }
    const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc((void *)p.lora_down, 0, (int)((size_t)p.R * K * 2), 0x00020000);
    auto slab_dma = [&](int rank0) { // ranks rank0 .. rank0 + 31 of this chunk's channels -> the tile region; ranks >= R lie beyond the descriptor's range and read as zero
#pragma unroll
        for (int i = 0; i < 8; i++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rl, (lds_void *)(W + i * 1024), 16, ldo[i & 3] + ((i >> 2) * 16 + rank0) * K * 2, 0, 0, 0);
    };

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
        // (one wave, in-order LDS: its reads below see its own writes; no workgroup barrier)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ---- 3. back in record layout: 8 bytes (half h) of piece 8 grp + tc of row r
#pragma unroll
        for (int grp = 0; grp < 2; grp++)
#pragma unroll
            for (int tc = 0; tc < 8; tc++) xv[grp][tc] = *(const lds_v2i *)(W + r * 256 + (((grp * 8 + tc) ^ (r & 15)) << 4) + 8 * h);
        if (p.R > 0) { // the tile is in registers: its LDS takes the first slab of lora_down while the groups below are quantised
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            slab_dma(0);
        }

        // ---- 4. the two groups of the chunk: the quantiser of quantize.hip, expression for expression
        uint8_t *dst = p.act + ((size_t)rt * KP + kp) * F6_CHUNK + (size_t)lane * 16;
#pragma unroll
        for (int grp = 0; grp < 2; grp++) {
            v16f ev, od; // elements 0,2 / 1,3 of the lane's eight 4-channel pieces = the two sources of the FP6 pack
            float amax = 0.f;
#pragma unroll
            for (int tc = 0; tc < 8; tc++) {
                v4f rs = {};
                if constexpr (SMOOTH) rs = *(const lds_v4f *)(W + QG_TILE_BYTES + (grp * 64 + 8 * tc + 4 * h) * 4);
                float xf[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    xf[e] = h2f(hfrom<T>((unsigned short)((unsigned)xv[grp][tc][e >> 1] >> (16 * (e & 1)))));
                    if constexpr (SMOOTH) xf[e] = smooth_div16<T>(xf[e], rs[e]);
                    amax = fmaxf(amax, fabsf(xf[e]));
                }
                ev[2 * tc] = xf[0]; ev[2 * tc + 1] = xf[2];
                od[2 * tc] = xf[1]; od[2 * tc + 1] = xf[3];
            }
            amax = fmaxf(amax, __shfl_xor(amax, 32));
            const float scale = amax * (1.0f / 7.0f);
            const float rscale = scale == 0.f ? 0.f : 1.0f / scale;
#pragma unroll
            for (int i = 0; i < 16; i++) { // NaN (a NaN element, or inf * 0 in a group holding inf) -> code 0, as in quantize.hip
                ev[i] = nan_to_zero(ev[i] * rscale);
                od[i] = nan_to_zero(od[i] * rscale);
            }
            const v6i pk = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(ev, od, 8.0f);
            if (grp == 0) {
                *reinterpret_cast<uint4 *>(dst) = make_uint4((unsigned)pk[0], (unsigned)pk[1], (unsigned)pk[2], (unsigned)pk[3]);
                *reinterpret_cast<uint2 *>(dst + F6_PLANE) = make_uint2((unsigned)pk[4], (unsigned)pk[5]);
            } else {
                *reinterpret_cast<uint2 *>(dst + F6_PLANE + 8) = make_uint2((unsigned)pk[0], (unsigned)pk[1]);
                *reinterpret_cast<uint4 *>(dst + 2 * F6_PLANE) = make_uint4((unsigned)pk[2], (unsigned)pk[3], (unsigned)pk[4], (unsigned)pk[5]);
            }
            // S image: [rt][kp][grp][32]; lane (r, h) writes group h
            if (h == grp) ((T *)p.ascales)[(((size_t)rt * KP + kp) * 2 + grp) * 32 + r] = f2h<T>(scale);
        }
    }

    // ---- 5. low rank, one 32-rank slab at a time: 8 MFMAs per wave (pieces 2q, 2q + 1 of every lane are k-slots 8h .. 8h + 7), the four waves' tiles
    //         parked in their own regions and summed by wave 0 in a fixed order; atomics only between workgroups
    for (int rank0 = 0; rank0 < p.R; rank0 += 32) { // block-uniform
        v16f acc;
#pragma unroll
        for (int j = 0; j < 16; j++) acc[j] = 0.f;
        if (active) {
            if (rank0 > 0) slab_dma(rank0); // (the barrier that closed the previous round has freed the region)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int grp = 0; grp < 2; grp++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int piece = grp * 8 + 2 * q;
                    const v2i b0 = *(const lds_v2i *)(W + r * 256 + ((piece ^ (r & 15)) << 4) + 8 * h);
                    const v2i b1 = *(const lds_v2i *)(W + r * 256 + (((piece + 1) ^ (r & 15)) << 4) + 8 * h);
                    const V8 a = __builtin_bit_cast(V8, v4i{xv[grp][2 * q][0], xv[grp][2 * q][1], xv[grp][2 * q + 1][0], xv[grp][2 * q + 1][1]});
                    const V8 b = __builtin_bit_cast(V8, v4i{b0[0], b0[1], b1[0], b1[1]});
                    acc = Half<DT>::mfma32(a, b, acc);
                }
        }
        *(lds_v16f *)(W + lane * 64) = acc; // (behind this wave's own slab reads: in-order LDS)
        __syncthreads();
        if (wave == 0) {
            const lds_u8 *B = (const lds_u8 *)lds + lane * 64;
            const v16f s = ((*(const lds_v16f *)(B) + *(const lds_v16f *)(B + QG_WAVE_BYTES)) + *(const lds_v16f *)(B + 2 * QG_WAVE_BYTES)) +
                           *(const lds_v16f *)(B + 3 * QG_WAVE_BYTES);
            if (rank0 + r < p.R) { // C layout: col (rank) = lane & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int m = rt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    lora_act_add(p.lora_act, (size_t)m * p.R + rank0 + r, s[i], p.mode);
                }
            }
        }
        __syncthreads();
    }
}

// clears lora_act ahead of a K-sliced launch (a kernel, not hipMemsetAsync: the launch may be recorded into a graph)
__global__ __launch_bounds__(256) void quantize_glu_clear(uint32_t *dst, size_t words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) dst[i] = 0u;
}

template <int DT, int ACT>
static int launch_quantize_glu(const svdq_quantize_glu_args *a, hipStream_t st) {
    const int KP = a->K / 128, slices = (KP + 3) / 4;
    const int q32 = a->lora_act_format != SVDQ_LORA_ACT_F32;
    const int mode = (slices > 1 ? 1 : 0) | (q32 ? 2 : 0);
    if (a->R > 0 && slices > 1 && !a->lora_act_zeroed) {
        const size_t words = (size_t)a->M_pad * a->R * (q32 ? 2 : 1);
        const size_t blocks = (words + 1023) / 1024;
        hipLaunchKernelGGL(quantize_glu_clear, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, (uint32_t *)a->lora_act, words);
    }
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
