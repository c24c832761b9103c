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
// svdq_gemm_mxfp4_qkv: the same loop under the RMSNorm + RoPE epilogue of a QKV projection, V optionally transposed (gemm_mxfp4_qkv_kernel below).
// svdq_gemm_mxfp4_glu_quant: the same loop under the GLU_QUANT epilogue of a gated projection, N = 2 Hd -- a workgroup's 128 tile columns are 64
// value rows and the 64 gate rows Hd further down the weight (gemm_mxfp4_glu_quant_kernel below).
#include <type_traits>

#include "glu_act.h"
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

// ---- the QKV variant: the attention projection of a block, N = 3 H 128.  Same loop, same low-rank-up MFMAs; the workgroup's 128 columns are one head
// of Q (bn < H), of K (bn < 2 H) or of V, block-uniformly.  With h32 = acc + bias:
//   Q, K   coef = rsqrt(sum_c h32_c^2 / 128 + 1e-6);  y_c = h32_c * ((coef * q_scale) * w_c);  pairs (2 j, 2 j + 1) rotated by the row's (sin, cos)_j;
//          one rounding.  A lane holds 64 of its row's 128 columns, so the sum of squares finishes in ONE exchange between the half-waves, and the
//          lane's columns 4 h + {0, 1} and 4 h + {2, 3} of every 8-column piece are whole pairs: the rotation crosses no lane.
//   V      round16(h32), the plain kernel's value -- into `out`, or with out_vt transposed: both stage buffers are dead behind the loop, so a wave
//          turns 32 rows x 128 columns at a time through its 12 KiB of them (column-major, 80 bytes a column: the 2-byte writes of the two
//          half-waves, four columns apart, fall into different banks) and stores 16 bytes = 8 consecutive tokens a lane, 64 contiguous bytes a column.
// The rotary table is pack_rotemb's: float (m >> 4) * 2048 + (c >> 3) * 128 + (m & 7) * 16 + ((c >> 1) & 3) * 4 + ((m >> 3) & 1) * 2 holds (sin, cos)
// of row m, pair c >> 1 -- two 8-byte loads per 8-column piece, rows up to M_pad (the table has them all).  The norm vector (32 registers, 16-bit)
// is loaded ahead of the bias; the rotary entries run one (row tile, block) = 16 registers ahead of the arithmetic, no further (as load_cols above).
struct Mxfp4QkvParams : Mxfp4GemmParams {
    const void *norm_q, *norm_k; // [128] 16-bit
    const float *rotary_emb;     // [M_pad][128]
    void *out_vt;                // [N / 3][ldvt] 16-bit or null
    long long ldvt;
    float q_scale;               // 1 = off
};

constexpr int MX_VT_COL = 80, MX_VT_WAVE = 2 * MX_STAGE / 4; // bytes a column (64 + 16), bytes of LDS a wave

template <int DT>
__global__ __launch_bounds__(256, 2) void gemm_mxfp4_qkv_kernel(Mxfp4QkvParams p) {
    using T = typename Half<DT>::T;
    using V8 = typename Half<DT>::V8;
#include "gemm_mxfp4_loop.inc"
    const int mw0 = m0 + wave * 64, heads = p.N / (3 * MX_TN);
    if (bn < 2 * heads) { // ---- Q or K
        const bool is_q = bn < heads;
        const T *nw = (const T *)(is_q ? p.norm_q : p.norm_k) + 4 * h;
        const float qs = is_q ? p.q_scale : 1.0f;
        u16x4 wv[4][4];
#pragma unroll
        for (int ni = 0; ni < 4; ni++)
#pragma unroll
            for (int g = 0; g < 4; g++) wv[ni][g] = *reinterpret_cast<const u16x4 *>(nw + ni * 32 + g * 8);
        const float *rrow[2];
#pragma unroll
        for (int mi = 0; mi < 2; mi++) {
            const unsigned m = (unsigned)(mw0 + mi * 32 + r);
            rrow[mi] = p.rotary_emb + (size_t)(m >> 4) * 2048 + (m & 7u) * 16u + ((m >> 3) & 1u) * 2u + 8 * h;
        }
        float2 rot[2][4][2]; // [block parity][piece][pair of the piece's lane columns]
        auto load_rot = [&](int blk) { // block blk = 4 mi + ni
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const float *rp = rrow[blk >> 2] + (4 * (blk & 3) + g) * 128;
                rot[blk & 1][g][0] = *reinterpret_cast<const float2 *>(rp);
                rot[blk & 1][g][1] = *reinterpret_cast<const float2 *>(rp + 4);
            }
        };
        load_rot(0);
        if (p.bias) {
#pragma unroll
            for (int ni = 0; ni < 4; ni++)
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const u16x4 bb = *reinterpret_cast<const u16x4 *>((const T *)p.bias + n0 + ni * 32 + g * 8 + 4 * h);
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float b = h2f(hfrom<T>(bb[e]));
                        acc[ni][0][4 * g + e] += b;
                        acc[ni][1][4 * g + e] += b;
                    }
                }
        }
        float coef[2];
#pragma unroll
        for (int mi = 0; mi < 2; mi++) {
            float s0 = 0.f, s1 = 0.f; // two chains: the 64 dependent fused multiply-adds of one would be the epilogue's critical path
#pragma unroll
            for (int ni = 0; ni < 4; ni++)
#pragma unroll
                for (int i = 0; i < 16; i += 2) {
                    s0 = __builtin_fmaf(acc[ni][mi][i], acc[ni][mi][i], s0);
                    s1 = __builtin_fmaf(acc[ni][mi][i + 1], acc[ni][mi][i + 1], s1);
                }
            float s = s0 + s1;
            s += __shfl_xor(s, 32); // the other 64 columns of the row (commutative: both halves hold the same sum)
            coef[mi] = __builtin_amdgcn_rsqf(s * (1.0f / 128.0f) + 1e-6f) * qs;
        }
#pragma unroll
        for (int mi = 0; mi < 2; mi++) {
            const int m = mw0 + mi * 32 + r;
            T *orow = (T *)p.out + (size_t)m * p.ldo + n0 + 4 * h;
#pragma unroll
            for (int ni = 0; ni < 4; ni++) {
                const int blk = 4 * mi + ni;
                if (blk + 1 < 8) load_rot(blk + 1);
                asm volatile("" ::: "memory");
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    float y[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) y[e] = acc[ni][mi][4 * g + e] * (coef[mi] * h2f(hfrom<T>(wv[ni][g][e])));
                    u16x4 o;
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        const float2 sc = rot[blk & 1][g][q]; // (sin, cos)
                        o[2 * q] = hbits(f2h<T>(__builtin_fmaf(y[2 * q], sc.y, -(y[2 * q + 1] * sc.x))));
                        o[2 * q + 1] = hbits(f2h<T>(__builtin_fmaf(y[2 * q], sc.x, y[2 * q + 1] * sc.y)));
                    }
                    if (m < p.M) *reinterpret_cast<u16x4 *>(orow + ni * 32 + g * 8) = o;
                }
            }
        }
        return;
    }
    // ---- V: the plain kernel's values
    const bool vt = p.out_vt != nullptr;
    if (vt) __syncthreads(); // every wave is through the last K-step's fragment reads: the stage buffers are free
    mx_lds_u8 *W = (mx_lds_u8 *)lds + wave * MX_VT_WAVE;
#pragma unroll
    for (int mi = 0; mi < 2; mi++) {
        const int m = mw0 + mi * 32 + r;
        T *orow = (T *)p.out + (size_t)m * p.ldo;
#pragma unroll
        for (int ni = 0; ni < 4; ni++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int c = ni * 32 + g * 8 + 4 * h;
                u16x4 bb = {0, 0, 0, 0}, o;
                if (p.bias) bb = *reinterpret_cast<const u16x4 *>((const T *)p.bias + n0 + c);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float v = acc[ni][mi][4 * g + e];
                    if (p.bias) v += h2f(hfrom<T>(bb[e]));
                    o[e] = hbits(f2h<T>(v));
                }
                if (!vt) {
                    if (m < p.M) *reinterpret_cast<u16x4 *>(orow + n0 + c) = o;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++) *(__attribute__((address_space(3))) unsigned short *)(W + (c + e) * MX_VT_COL + 2 * r) = o[e];
                }
            }
        if (!vt) continue;
        __syncthreads(); // (the waves share nothing here: the barrier orders a wave's own lanes' writes ahead of its reads, and costs three a tile)
        const int mq = mw0 + mi * 32 + 8 * (lane & 3); // the lane's 8 tokens
        const mx_lds_u8 *src = W + (lane >> 2) * MX_VT_COL + 16 * (lane & 3);
        T *dst = (T *)p.out_vt + (size_t)(n0 - 2 * heads * MX_TN + (lane >> 2)) * p.ldvt + mq;
        const int mt = m0 + __builtin_amdgcn_readfirstlane(wave) * 64 + mi * 32; // the row tile's first row, as a scalar: the two branches are wave-uniform
        if (mt + 32 <= p.M) { // all 32 rows are tokens: eight reads, then eight stores
            v4i t[8];
#pragma unroll
            for (int j = 0; j < 8; j++) t[j] = *(const mx_lds_v4i *)(src + 16 * j * MX_VT_COL);
#pragma unroll
            for (int j = 0; j < 8; j++) *reinterpret_cast<v4i *>(dst + (size_t)16 * j * p.ldvt) = t[j];
        } else if (mt < p.M) { // the row tile M ends in: whole pieces as above, the piece that holds row M token by token
#pragma unroll 1
            for (int j = 0; j < 8; j++) {
                const v4i t = *(const mx_lds_v4i *)(src + 16 * j * MX_VT_COL);
                T *d = dst + (size_t)16 * j * p.ldvt;
                if (mq + 8 <= p.M) *reinterpret_cast<v4i *>(d) = t;
                else {
#pragma unroll
                    for (int e = 0; e < 8; e++)
                        if (mq + e < p.M) d[e] = hfrom<T>((unsigned short)((unsigned)t[e >> 1] >> (16 * (e & 1))));
                }
            }
        }
        if (mi == 0) __syncthreads(); // the reads are through before the second row tile overwrites the columns
    }
}

// ---- the GLU_QUANT variant: the gated projection of a SwiGLU / GEGLU feed-forward, weight [2 Hd][K] with the value half in rows [0, Hd) and the
// gate half in rows [Hd, 2 Hd) (p.N = 2 Hd).  Same loop, same low-rank-up MFMAs, but the workgroup's 128 tile columns are PAIRED (MX_WBASE, MX_WSKIP):
// accumulator tiles ni = 0, 1 are value rows 64 bn .. 64 bn + 63, tiles ni = 2, 3 the gate rows Hd + 64 bn .. Hd + 64 bn + 63, so value c and gate c
// of a row are the same element of tiles ni and ni + 2 of the same lane: the product crosses no lane and needs no LDS.  With h32 = acc + bias
// (the bias by weight row):
//   v16 = round16(h32 value), g16 = round16(h32 gate)     the plain kernel's output columns
//   a = round16(act(g16)),  x = round16(v16 * a)           act = glu_silu | glu_gelu (glu_act.h): svdq_quantize_glu_halves's rounding points; rows >= M: 0
//   the MXFP4 block quantiser on round16(x * rcp(smooth_next))   -> qout [M_pad][Hd / 2], oscales [Hd / 128][M_pad] dwords; x -> out (OUT16)
//   lora_act_out[m, :] += x[m, 64 bn .. 64 bn + 63] @ down_next[64 bn .. 64 bn + 63, :]    (fp32 atomics, the last thing issued)
// The 64 x-channels of a workgroup are HALF a K-step of the next GEMM: 32 code bytes a row (one 16-byte store a lane: half h keeps block h) and two
// of the four scale bytes of dword (bn >> 1, m) -- one 16-bit store into half bn & 1 of it; the neighbouring tile completes the dword.
// A block nb takes tiles nb and nb + 2 out of the accumulator and leaves 8 packed registers a row tile: every finished block frees 48 of 64.
template <int DT, int ACT, bool OUT16>
__global__ __launch_bounds__(256, 2) void gemm_mxfp4_glu_quant_kernel(Mxfp4GeluQuantParams p) {
    using T = typename Half<DT>::T;
    using V8 = typename Half<DT>::V8;
    const int Hd = p.N >> 1;
#define MX_WBASE (bn * 64)
#define MX_WSKIP(c) (((c) >> 6) ? Hd - 64 : 0)
#include "gemm_mxfp4_loop.inc"
    const int mw0 = m0 + wave * 64; // the wave's rows mw0 + 32 mi + r, all < M_pad
    const int c0 = bn * 64 + 4 * h; // the lane's x channels: c0 + 32 nb + 8 g + e
    unsigned xp[2][2][8];           // x, two 16-bit values a register in the accumulator's order
    unsigned pc[2][2][2], sb2[2] = {0, 0};
#pragma unroll
    for (int nb = 0; nb < 2; nb++) {
        if (p.bias) { // value and gate bias of the lane's 16 channels of block nb: h32
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const u16x4 bv = *reinterpret_cast<const u16x4 *>((const T *)p.bias + c0 + 32 * nb + 8 * g);
                const u16x4 bg = *reinterpret_cast<const u16x4 *>((const T *)p.bias + Hd + c0 + 32 * nb + 8 * g);
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int mi = 0; mi < 2; mi++) {
                        acc[nb][mi][4 * g + e] += h2f(hfrom<T>(bv[e]));
                        acc[nb + 2][mi][4 * g + e] += h2f(hfrom<T>(bg[e]));
                    }
            }
        }
        float rs[16]; // 1 / smooth_next; without smoothing rcp(1) = 1 exactly and x * 1 = x, the quantiser's un-smoothed path
#pragma unroll
        for (int i = 0; i < 16; i++) rs[i] = 1.0f;
        if (p.smooth_next) {
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const u16x4 sv = *reinterpret_cast<const u16x4 *>((const T *)p.smooth_next + c0 + 32 * nb + 8 * g);
#pragma unroll
                for (int e = 0; e < 4; e++) rs[4 * g + e] = __builtin_amdgcn_rcpf(h2f(hfrom<T>(sv[e])));
            }
        }
#pragma unroll
        for (int mi = 0; mi < 2; mi++) {
            const bool live = mw0 + mi * 32 + r < p.M; // a padding row holds bias * act(bias): cut to zero, as the quantiser leaves it
            float v[16], amax = 0.f;
#pragma unroll
            for (int i = 0; i < 16; i += 2) {
                const f32x2_t v16 = round16_pair<T>(acc[nb][mi][i], acc[nb][mi][i + 1]);
                const f32x2_t g16 = round16_pair<T>(acc[nb + 2][mi][i], acc[nb + 2][mi][i + 1]);
                f32x2_t a;
                if constexpr (ACT == SVDQ_GLU_SILU) a = round16_pair<T>(glu_silu(g16[0]), glu_silu(g16[1]));
                else a = round16_pair<T>(glu_gelu(g16[0]), glu_gelu(g16[1]));
                f32x2_t t = round16_pair<T>(v16[0] * a[0], v16[1] * a[1]); // (the product of two 16-bit values is exact in fp32: one rounding)
                if (!live) t = f32x2_t{0.f, 0.f};
                xp[nb][mi][i >> 1] = (unsigned)hbits(f2h<T>(t[0])) | (unsigned)hbits(f2h<T>(t[1])) << 16; // (exact: t is a 16-bit value)
                asm volatile("" : "+v"(xp[nb][mi][i >> 1])); // (pinned here, as g in the GELU_QUANT kernel: sunk to its use, the pack keeps both fp32 values alive)
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    v[i + e] = smooth_div16<T>(t[e], rs[i + e]);
                    amax = mx_amax_acc(amax, v[i + e]);
                }
            }
            const unsigned sb = mx_block_byte<T>(amax);
            MX_BLOCK_CODES(v, sb, pc[mi][nb]);
            sb2[mi] |= sb << (8 * nb);
            if constexpr (OUT16) {
                if (live) {
                    T *orow = (T *)p.out + (size_t)(mw0 + mi * 32 + r) * p.ldo + c0 + 32 * nb;
#pragma unroll
                    for (int g = 0; g < 4; g++) *reinterpret_cast<uint2 *>(orow + 8 * g) = make_uint2(xp[nb][mi][2 * g], xp[nb][mi][2 * g + 1]);
                }
            }
            __builtin_amdgcn_sched_barrier(0); // one (block, row tile) at a time, as in the GELU_QUANT kernel
        }
    }
    // the row's 32 code bytes: the halves trade pieces so that lane h keeps block h -- dword q = piece q of half 0 | piece q of half 1 << 16 (as
    // mx_trade_halves, for two blocks) -- and stores its 16 bytes; half 0 stores the two scale bytes
#pragma unroll
    for (int mi = 0; mi < 2; mi++) {
        const int m = mw0 + mi * 32 + r;
        unsigned dw[4];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const unsigned own = h ? pc[mi][1][t] : pc[mi][0][t];
            const unsigned oth = (unsigned)__shfl_xor((int)(h ? pc[mi][0][t] : pc[mi][1][t]), 32);
            const unsigned a = h ? oth : own, bq = h ? own : oth; // a: half 0's pieces, bq: half 1's
            dw[2 * t] = (a & 0xffffu) | (bq << 16);
            dw[2 * t + 1] = (a >> 16) | (bq & 0xffff0000u);
        }
        *reinterpret_cast<uint4 *>(p.qout + (size_t)m * (Hd / 2) + bn * 32 + 16 * h) = make_uint4(dw[0], dw[1], dw[2], dw[3]);
        if (h == 0) reinterpret_cast<unsigned short *>(p.oscales + (size_t)(bn >> 1) * p.M_pad + m)[bn & 1] = (unsigned short)sb2[mi];
    }
    // the next layer's low-rank down projection on the un-smoothed x, 32 ranks a pass on the 16-bit 32x32x16 MFMA: operands, order and atomics as in
    // the GELU_QUANT kernel, over the tile's 64 channels (two blocks x two k-slots of 16)
    const int mws = m0 + __builtin_amdgcn_readfirstlane(wave) * 64; // = mw0, as a scalar
    for (int t2 = 0; t2 < p.R_next; t2 += 32) {
        const bool rank_live = t2 + r < p.R_next; // a half-filled 32-rank tile: zeros beyond R_next
        V8 wv[2][2];
#pragma unroll
        for (int nb = 0; nb < 2; nb++)
#pragma unroll
            for (int q = 0; q < 2; q++) {
                u16x4 w0 = {0, 0, 0, 0}, w1 = {0, 0, 0, 0};
                if (rank_live) {
                    const T *src = (const T *)p.down_next + (size_t)(t2 + r) * Hd + c0 + nb * 32 + q * 16;
                    w0 = *reinterpret_cast<const u16x4 *>(src);
                    w1 = *reinterpret_cast<const u16x4 *>(src + 8);
                }
#pragma unroll
                for (int j = 0; j < 4; j++) { wv[nb][q][j] = hfrom<T>(w0[j]); wv[nb][q][4 + j] = hfrom<T>(w1[j]); }
            }
        v16f d[2];
#pragma unroll
        for (int mi = 0; mi < 2; mi++)
#pragma unroll
            for (int i = 0; i < 16; i++) d[mi][i] = 0.f;
#pragma unroll
        for (int nb = 0; nb < 2; nb++)
#pragma unroll
            for (int q = 0; q < 2; q++)
#pragma unroll
                for (int mi = 0; mi < 2; mi++) {
                    const V8 xv = __builtin_bit_cast(V8, v4i{(int)xp[nb][mi][4 * q], (int)xp[nb][mi][4 * q + 1], (int)xp[nb][mi][4 * q + 2], (int)xp[nb][mi][4 * q + 3]});
                    d[mi] = Half<DT>::mfma32(xv, wv[nb][q], d[mi]);
                }
#pragma unroll
        for (int mi = 0; mi < 2; mi++) {
            if (!rank_live || mws + mi * 32 >= p.M) continue;
            float *base = p.lora_act_out + (size_t)(mws + mi * 32) * p.R_next; // D element i: row (i & 3) + 8 (i >> 2) + 4 h, column (rank) r
            const unsigned off = (unsigned)(4 * h * p.R_next + t2 + r);
#pragma unroll
            for (int i = 0; i < 16; i++) unsafeAtomicAdd(base + (size_t)((i & 3) + 8 * (i >> 2)) * p.R_next + off, d[mi][i]);
        }
    }
}

// clears lora_act_out ahead of the GELU_QUANT / GLU_QUANT launch (a kernel, not hipMemsetAsync: the launch may be recorded into a graph)
static __global__ __launch_bounds__(256) void gemm_mxfp4_clear(uint32_t *dst, size_t words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) dst[i] = 0u;
}

} // namespace svdq

using namespace svdq;

// what the entries check of the fields they share (A: svdq_gemm_mxfp4_args, svdq_gemm_mxfp4_gelu_quant_args, svdq_gemm_mxfp4_glu_quant_args or
// svdq_gemm_mxfp4_qkv_args); 0 or the error code, nothing is launched.  `rows`: the rows the grid covers; `out_div`: `out` has N / out_div columns.
// fills the kernel's parameters
template <typename A> static int mx_gemm_validate(const A *a, const char *fn, bool need_out, int rows, Mxfp4GemmParams &p, long long &grid, int out_div = 1) {
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
    if (a->out && (a->ldo < a->N / out_div || a->ldo % 4)) { set_error("%s: ldo=%d must be >= %s and a multiple of 4", fn, a->ldo, out_div == 1 ? "N" : "N / 2"); return SVDQ_E_INVALID; }
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

extern "C" int svdq_gemm_mxfp4_qkv(const svdq_gemm_mxfp4_qkv_args *a, void *stream) {
    const char *fn = "svdq_gemm_mxfp4_qkv";
    Mxfp4QkvParams p;
    long long grid;
    if (const int rc = mx_gemm_validate(a, fn, true, a ? a->M : 0, p, grid)) return rc;
    if (a->N % (3 * MX_TN)) { set_error("%s: N=%d must be a multiple of 384 (3 x heads x 128)", fn, a->N); return SVDQ_E_INVALID; }
    if (!a->norm_q || !a->norm_k || !a->rotary_emb) { set_error("%s: norm_q, norm_k and rotary_emb are required", fn); return SVDQ_E_INVALID; }
    if (((uintptr_t)a->norm_q | (uintptr_t)a->norm_k | (uintptr_t)a->rotary_emb) & 7) { set_error("%s: norm_q, norm_k and rotary_emb must be 8-byte aligned", fn); return SVDQ_E_INVALID; }
    if (a->out_vt && (((uintptr_t)a->out_vt & 15) || a->ldvt < a->M || a->ldvt % 8)) {
        set_error("%s: out_vt must be 16-byte aligned with ldvt=%d >= M=%d a multiple of 8", fn, a->ldvt, a->M);
        return SVDQ_E_INVALID;
    }
    if (!(a->q_scale >= 0.f) || a->q_scale > 3.0e38f) { set_error("%s: q_scale must be finite and >= 0 (0 = off)", fn); return SVDQ_E_INVALID; }
    // (addressing reach: the table's, out's and out_vt's row addresses are formed in 64 bits -- nothing beyond what the shared checks hold)
    p.norm_q = a->norm_q; p.norm_k = a->norm_k; p.rotary_emb = (const float *)a->rotary_emb; p.out_vt = a->out_vt; p.ldvt = a->ldvt;
    p.q_scale = a->q_scale == 0.f ? 1.0f : a->q_scale;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == SVDQ_BF16) hipLaunchKernelGGL((gemm_mxfp4_qkv_kernel<SVDQ_BF16>), dim3((unsigned)grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((gemm_mxfp4_qkv_kernel<SVDQ_FP16>), dim3((unsigned)grid), dim3(256), 0, st, p);
    return hip_check(hipGetLastError(), "svdq_gemm_mxfp4_qkv launch");
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

extern "C" int svdq_gemm_mxfp4_glu_quant(const svdq_gemm_mxfp4_glu_quant_args *a, void *stream) {
    const char *fn = "svdq_gemm_mxfp4_glu_quant";
    Mxfp4GeluQuantParams p;
    long long grid; // M_pad / 256 * N / 128 = M_pad / 256 * Hd / 64
    if (const int rc = mx_gemm_validate(a, fn, false, a ? a->M_pad : 0, p, grid, 2)) return rc;
    if (a->N % 256) { set_error("%s: N=%d must be 2 * Hd with Hd a multiple of 128", fn, a->N); return SVDQ_E_INVALID; }
    if (a->act_fn != SVDQ_GLU_SILU && a->act_fn != SVDQ_GLU_GELU_ERF) { set_error("%s: unknown act_fn %d", fn, a->act_fn); return SVDQ_E_INVALID; }
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
    const int variant = (a->dtype == SVDQ_FP16 ? 4 : 0) | (a->act_fn == SVDQ_GLU_GELU_ERF ? 2 : 0) | (a->out ? 1 : 0);
    switch (variant) {
    case 0: hipLaunchKernelGGL((gemm_mxfp4_glu_quant_kernel<SVDQ_BF16, SVDQ_GLU_SILU, false>), g, b, 0, st, p); break;
    case 1: hipLaunchKernelGGL((gemm_mxfp4_glu_quant_kernel<SVDQ_BF16, SVDQ_GLU_SILU, true>), g, b, 0, st, p); break;
    case 2: hipLaunchKernelGGL((gemm_mxfp4_glu_quant_kernel<SVDQ_BF16, SVDQ_GLU_GELU_ERF, false>), g, b, 0, st, p); break;
    case 3: hipLaunchKernelGGL((gemm_mxfp4_glu_quant_kernel<SVDQ_BF16, SVDQ_GLU_GELU_ERF, true>), g, b, 0, st, p); break;
    case 4: hipLaunchKernelGGL((gemm_mxfp4_glu_quant_kernel<SVDQ_FP16, SVDQ_GLU_SILU, false>), g, b, 0, st, p); break;
    case 5: hipLaunchKernelGGL((gemm_mxfp4_glu_quant_kernel<SVDQ_FP16, SVDQ_GLU_SILU, true>), g, b, 0, st, p); break;
    case 6: hipLaunchKernelGGL((gemm_mxfp4_glu_quant_kernel<SVDQ_FP16, SVDQ_GLU_GELU_ERF, false>), g, b, 0, st, p); break;
    default: hipLaunchKernelGGL((gemm_mxfp4_glu_quant_kernel<SVDQ_FP16, SVDQ_GLU_GELU_ERF, true>), g, b, 0, st, p); break;
    }
    return hip_check(hipGetLastError(), "svdq_gemm_mxfp4_glu_quant launch");
}
