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
#include <type_traits>

#include "svdq_common.h"

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
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * MX_STAGE];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int r = lane & 31, h = lane >> 5;
    const int TN = p.N / MX_TN;
    const int bm = blockIdx.x / TN, bn = blockIdx.x % TN;
    const int m0 = bm * MX_TM, n0 = bn * MX_TN;
    const int KB = p.K / 2, KS = p.K / 128;

    // ---- DMA plan: position pos = 64 i + lane of a tile holds row pos >> 2, slot pos & 3 = block (slot ^ ((row >> 2) & 3)); the A tile is 16
    //      wave instructions (4 a wave), the B tile 8 (2 a wave).  Offsets are range-checked 32-bit byte offsets (validated on the host).
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void *)p.act, 0, (int)((size_t)p.M_pad * KB), 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void *)p.wgt, 0, (int)((size_t)p.N * KB), 0x00020000);
    unsigned va[4], vw[2];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned pos = (unsigned)(wave * 4 + j) * 64u + lane, row = pos >> 2, blk = (pos & 3u) ^ ((row >> 2) & 3u);
        va[j] = (unsigned)(m0 + row) * (unsigned)KB + blk * 16u;
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const unsigned pos = (unsigned)(wave * 2 + j) * 64u + lane, row = pos >> 2, blk = (pos & 3u) ^ ((row >> 2) & 3u);
        vw[j] = (unsigned)(n0 + row) * (unsigned)KB + blk * 16u;
    }
    auto stage_dma = [&](int ks, int buf) {
        mx_lds_u8 *S = (mx_lds_u8 *)lds + buf * MX_STAGE;
#pragma unroll
        for (int j = 0; j < 4; j++) __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (mx_lds_void *)(S + (wave * 4 + j) * 1024), 16, va[j], ks * 64, 0, 0);
#pragma unroll
        for (int j = 0; j < 2; j++) __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (mx_lds_void *)(S + MX_A_BYTES + (wave * 2 + j) * 1024), 16, vw[j], ks * 64, 0, 0);
    };
    // the scale dwords of K-step ks: lane (r, h) takes those of its own rows / columns; behind the step's wait it moves block h to byte 0 (block 2 + h to byte 2)
    const uint32_t *sa_ptr = p.ascales + m0 + wave * 64 + r, *sw_ptr = p.wscales + n0 + r;
    auto load_scales = [&](int ks, unsigned (&sa)[2], unsigned (&sw)[4]) {
#pragma unroll
        for (int mi = 0; mi < 2; mi++) sa[mi] = sa_ptr[(size_t)ks * p.M_pad + 32 * mi];
#pragma unroll
        for (int ni = 0; ni < 4; ni++) sw[ni] = sw_ptr[(size_t)ks * p.N + 32 * ni];
    };

    v16f acc[4][2];
#pragma unroll
    for (int ni = 0; ni < 4; ni++)
#pragma unroll
        for (int mi = 0; mi < 2; mi++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[ni][mi][i] = 0.f;

    // fragment addresses inside a stage: rows 64 wave + 32 mi + r of A, 32 ni + r of B; (row >> 2) & 3 = (r >> 2) & 3 for both
    const unsigned sw3 = ((unsigned)r >> 2) & 3u;
    const unsigned fa = (unsigned)(wave * 64 + r) * 64u, fb = (unsigned)MX_A_BYTES + (unsigned)r * 64u;

    unsigned sa_n[2], sw_n[4];
    load_scales(0, sa_n, sw_n);
    stage_dma(0, 0);
    for (int ks = 0; ks < KS; ks++) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's part of step ks has landed ...
        __syncthreads();                                 // ... and everybody's; every wave is done reading the other buffer
        unsigned sa[2], sw[4];
#pragma unroll
        for (int i = 0; i < 2; i++) { asm volatile("" : "+v"(sa_n[i])); sa[i] = sa_n[i] >> (8 * h); } // (pinned behind the wait: hoisted into the previous step, the
#pragma unroll
        for (int i = 0; i < 4; i++) { asm volatile("" : "+v"(sw_n[i])); sw[i] = sw_n[i] >> (8 * h); } //  shifts put an s_waitcnt vmcnt(6) between that step's MFMAs)
        if (ks + 1 < KS) { // block-uniform; the scale loads first, so that a wait for them leaves the six DMA instructions in flight: hipcc copies the loaded
                           // dwords into their loop-carried registers behind the step's 10th to 14th MFMA (s_waitcnt vmcnt(11) / (9) / (6))
            load_scales(ks + 1, sa_n, sw_n);
            stage_dma(ks + 1, (ks + 1) & 1);
        }
        const mx_lds_u8 *S = (const mx_lds_u8 *)lds + (ks & 1) * MX_STAGE;
        auto extent = [&](auto kk_c) { // one MFMA K-extent of 64 channels: the lane's block is 2 kk + h (kk is an immediate: op_sel)
            constexpr int kk = decltype(kk_c)::value;
            const unsigned slot = (((unsigned)(2 * kk + h)) ^ sw3) << 4;
            v8i a[2], b[4];
#pragma unroll
            for (int mi = 0; mi < 2; mi++) {
                const v4i t = *(const mx_lds_v4i *)(S + fa + mi * 2048 + slot);
                a[mi] = v8i{t[0], t[1], t[2], t[3], 0, 0, 0, 0};
            }
#pragma unroll
            for (int ni = 0; ni < 4; ni++) {
                const v4i t = *(const mx_lds_v4i *)(S + fb + ni * 2048 + slot);
                b[ni] = v8i{t[0], t[1], t[2], t[3], 0, 0, 0, 0};
            }
#pragma unroll
            for (int ni = 0; ni < 4; ni++)
#pragma unroll
                for (int mi = 0; mi < 2; mi++) // D[n][m]: the weights are the first operand, so a lane ends up with 4 neighbouring columns of one row
                    acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b[ni], a[mi], acc[ni][mi], 4, 4, 2 * kk, (int)sw[ni], 2 * kk, (int)sa[mi]);
        };
        extent(std::integral_constant<int, 0>{});
        extent(std::integral_constant<int, 1>{});
    }

    // ---- epilogue.  Low rank on the 16-bit MFMA, 16 ranks at a time in ascending order, with gemm_w4a4's rounding point: round16(lora_act * scale)
    const int Rr = p.R;
    if (Rr > 0) {
        const float *la_base = p.lora_act + (size_t)(m0 + wave * 64 + r) * Rr + 8 * h;
        const T *lu_base = (const T *)p.lora_up + (size_t)(n0 + r) * Rr + 8 * h;
        for (int rc = 0; rc < Rr; rc += 16) {
            const float sc = p.lora_scales[rc >> 4];
            V8 la[2], lu[4];
#pragma unroll
            for (int mi = 0; mi < 2; mi++) {
                const v4f x0 = *reinterpret_cast<const v4f *>(la_base + (size_t)mi * 32 * Rr + rc);
                const v4f x1 = *reinterpret_cast<const v4f *>(la_base + (size_t)mi * 32 * Rr + rc + 4);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    la[mi][j] = f2h<T>(sc == 1.0f ? x0[j] : x0[j] * sc);
                    la[mi][4 + j] = f2h<T>(sc == 1.0f ? x1[j] : x1[j] * sc);
                }
            }
#pragma unroll
            for (int ni = 0; ni < 4; ni++) lu[ni] = *reinterpret_cast<const V8 *>(lu_base + (size_t)ni * 32 * Rr + rc);
#pragma unroll
            for (int ni = 0; ni < 4; ni++)
#pragma unroll
                for (int mi = 0; mi < 2; mi++) acc[ni][mi] = Half<DT>::mfma32(lu[ni], la[mi], acc[ni][mi]);
        }
    }
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

} // namespace svdq

using namespace svdq;

extern "C" int svdq_gemm_mxfp4(const svdq_gemm_mxfp4_args *a, void *stream) {
    if (!a) { set_error("svdq_gemm_mxfp4: args is NULL"); return SVDQ_E_INVALID; }
    if (!a->act || !a->wgt || !a->ascales || !a->wscales || !a->out) { set_error("svdq_gemm_mxfp4: act, wgt, ascales, wscales and out are required"); return SVDQ_E_INVALID; }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("svdq_gemm_mxfp4: unknown dtype %d", a->dtype); return SVDQ_E_INVALID; }
    if (a->M <= 0 || a->M_pad < a->M || a->M_pad % 256) {
        set_error("svdq_gemm_mxfp4: need 0 < M=%d <= M_pad=%d and M_pad %% 256 == 0", a->M, a->M_pad);
        return SVDQ_E_INVALID;
    }
    if (a->N <= 0 || a->N % 128) { set_error("svdq_gemm_mxfp4: N=%d must be a positive multiple of 128", a->N); return SVDQ_E_INVALID; }
    if (a->K <= 0 || a->K % 128) { set_error("svdq_gemm_mxfp4: K=%d must be a positive multiple of 128", a->K); return SVDQ_E_INVALID; }
    if (a->ldo < a->N || a->ldo % 4) { set_error("svdq_gemm_mxfp4: ldo=%d must be >= N and a multiple of 4", a->ldo); return SVDQ_E_INVALID; }
    if (a->R < 0 || a->R % 16 || a->R > 16 * MX_MAX_LORA_TILES) { set_error("svdq_gemm_mxfp4: R=%d must be a multiple of 16 in [0, 256]", a->R); return SVDQ_E_INVALID; }
    if (a->R > 0 && (!a->lora_act_in || !a->lora_up)) { set_error("svdq_gemm_mxfp4: R > 0 needs lora_act_in and lora_up"); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->act | (uintptr_t)a->wgt | (uintptr_t)a->lora_act_in | (uintptr_t)a->lora_up) & 15) {
        set_error("svdq_gemm_mxfp4: act, wgt, lora_act_in and lora_up must be 16-byte aligned");
        return SVDQ_E_INVALID;
    }
    if (((uintptr_t)a->out | (uintptr_t)a->bias) & 7) { set_error("svdq_gemm_mxfp4: out and bias must be 8-byte aligned"); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->ascales | (uintptr_t)a->wscales) & 3) { set_error("svdq_gemm_mxfp4: ascales and wscales must be 4-byte aligned"); return SVDQ_E_INVALID; }
    // addressing reach: the operand tiles are fetched through buffer descriptors with 32-bit byte offsets
    if ((long long)a->M_pad * (a->K / 2) > 0x7fffffffLL || (long long)a->N * (a->K / 2) > 0x7fffffffLL) {
        set_error("svdq_gemm_mxfp4: M_pad * K / 2 = %lld or N * K / 2 = %lld bytes exceed the 2147483647 the tile loads reach", (long long)a->M_pad * (a->K / 2),
                  (long long)a->N * (a->K / 2));
        return SVDQ_E_UNSUPPORTED;
    }
    const long long grid = (long long)((a->M + MX_TM - 1) / MX_TM) * (a->N / MX_TN);
    if (grid > 0x7fffffffLL) { set_error("svdq_gemm_mxfp4: M=%d x N=%d needs more than 2147483647 workgroups", a->M, a->N); return SVDQ_E_UNSUPPORTED; }
    Mxfp4GemmParams p{(const uint8_t *)a->act, (const uint8_t *)a->wgt, (const uint32_t *)a->ascales, (const uint32_t *)a->wscales, a->bias, a->lora_up,
                      (const float *)a->lora_act_in, a->out, a->ldo, a->M, a->M_pad, a->N, a->K, a->R, {}};
    for (int i = 0; i < MX_MAX_LORA_TILES; i++) p.lora_scales[i] = (a->lora_scales && i < a->R / 16) ? a->lora_scales[i] : 1.0f;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == SVDQ_BF16) hipLaunchKernelGGL((gemm_mxfp4_kernel<SVDQ_BF16>), dim3((unsigned)grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((gemm_mxfp4_kernel<SVDQ_FP16>), dim3((unsigned)grid), dim3(256), 0, st, p);
    return hip_check(hipGetLastError(), "svdq_gemm_mxfp4 launch");
}
