// svdq_pulid_ca: the identity cross-attention of PuLID (reference: nunchaku/models/pulid/encoders_transformer.py PerceiverAttentionCA --
// two LayerNorms, three dense GEMMs and a 16-bit softmax in torch ops) with both dense GEMMs FOLDED into the keys and values.  K and V depend
// on the identity embeddings only, and a head has at most 32 identity tokens against a head dimension of 128, so with n = LN(hidden) (no affine)
//
//   scores_h = n . A_h + c_h,   A_h = diag(w2) Wq_h^T K_h^T / sqrt(128)  [C, 32],   c_h = b2 . (Wq_h^T K_h^T / sqrt(128))
//   out      = sum_h softmax(scores_h) . B_h,   B_h = V_h Wo_h^T  [32, C]
//
// an attention whose H heads share ONE query -- the hidden row itself -- over J = H * 32 keys a_fold [J, C] and values b_fold [J, C], the outputs
// summed over the heads.  The LayerNorm lives in the score epilogue: s = rstd (x . a - mean colsum(a)) + c.  
//
// Two launches of ONE 16-bit MFMA tile loop (pulid_tile_kernel), D^T[a][t] = sum_k A[a][k] B[t][k] on the 32x32x16 MFMA in the S^T formulation of
// attn_frag.h (ip_attention.hip's header comment derives the operand layouts; they are the verified ones):
//   * scores:  A = a_fold (128 keys x 128 channels per step, a straight 16-byte copy into LDS), B = rows of x read from memory into registers,
//     K = C.  A 32-key accumulator tile is exactly one head: lane (lr, h) holds 16 of row lr's 32 scores of that head, lane ^ 32 the other 16, so
//     the softmax is register work and one lane exchange.  It writes probs [T, J] 16-bit.
//   * output:  A = b_fold^T (128 channels x 128 keys per step; b_fold is key-major, so the staging transposes 8x8 blocks in registers:
//     attn_frag.h's transpose8x8_piece), B = rows of probs, K = J.  It writes out [T, C].
// A workgroup is 4 waves on a 64-row x 128-column tile of D (wave: 32 rows x 64 columns, two accumulator tiles); the A tile of one step is 32 KiB
// of LDS in ip_attention.hip's K layout (256-byte rows, 16-byte piece p of row r at column p ^ (r & 15): conflict-free ds_read_b128); one
// ds_read_b128 per MFMA.  The next step's A pieces and B fragments are loaded into registers while the current step's MFMAs run.
// Why two launches and not one that keeps P in registers: a single launch gives every workgroup ALL of a_fold and b_fold (6 MB at C = 3072) to
// stream for its few rows; two launches let a workgroup stream one 128-column slice of one of them, and probs [T, 512] is 4 MB at T = 4096.
//
// Arithmetic (include/svdq_amd.h states the contract; tests/pulid_ref.py restates it): everything behind the MFMA accumulators is plain fp32
// multiplies, adds and one IEEE division in a fixed order (-ffp-contract=off), the exponential included (pulid_exp: no v_exp_f32), so a CPU
// restatement of the two epilogues is bit-equal.  No atomics; every element is produced by one lane: two calls are bit-equal, and a row's result
// depends on neither T nor the row's place in a tile (an MFMA column depends on its own B fragment only).
//   * keys n >= N of a head: their A rows are zeros in LDS (never read from memory), their scores -inf, their probabilities +0.
//   * rows at or beyond T: the loads are clamped to row T - 1, the stores skipped.
#include "svdq_common.h"
#include "attn_frag.h"

namespace svdq {

struct PulidParams {
    const uint16_t *a;  // the A operand's source: a_fold (scores) or b_fold (output), [J, C] row-major
    const uint16_t *b;  // the B operand's source: x (scores) or probs (output), rows of ldb elements
    const float *stats, *colsum, *cbias;
    uint16_t *dst;      // probs [T, J] (scores) or out [T, ldo] (output)
    float *dbg;         // optional fp32 copy of the accumulators: [T, J] (scores) or [T, C] (output)
    int ldb, ldd;       // row strides of b and dst in elements
    int T, C, J, N;
    int groups;         // 128-column groups of D: J / 128 (scores) or C / 128 (output)
    float out_scale;
};

constexpr int PCA_NW = 4;        // waves per workgroup: 2 (rows) x 2 (columns)
constexpr int PCA_ROWS = 64;     // rows of x / probs per workgroup
constexpr int PCA_COLS = 128;    // columns of D (keys, or output channels) per workgroup
constexpr int PCA_KSTEP = 128;   // K per step: one 256-byte LDS row
constexpr int PCA_LDS = PCA_COLS * PCA_KSTEP * 2;
constexpr float PCA_EXP_FLOOR = -80.0f; // exp(d) for d below this is +0: every non-zero e / sum(e) stays a normal fp32 number

// exp(d) for d <= 0 from plain fp32 operations, each rounded on its own: n = rint(d log2(e)), r = d - n ln2 (two-piece), a degree-7 Taylor
// polynomial by Horner, the exponent added to the bits (the result is normal: d >= -80).  |relative error| < 2^-22; what matters is that
// tests/pulid_ref.py forms the same bits.
__device__ __forceinline__ float pulid_exp(float d0) {
    const float d = fmaxf(d0, -100.0f); // (-inf of a masked key: the arithmetic below stays finite, the result is +0 either way)
    const float t = d * 1.4426950408889634f;
    const float n = __builtin_rintf(t);
    float r = d - n * 0.693145751953125f;
    r = r - n * 1.428606765330187e-06f;
    float p = 1.0f / 5040.0f;
    p = p * r + 1.0f / 720.0f;
    p = p * r + 1.0f / 120.0f;
    p = p * r + 1.0f / 24.0f;
    p = p * r + 1.0f / 6.0f;
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    const float e = __builtin_bit_cast(float, __builtin_bit_cast(int, p) + (int)n * (1 << 23));
    return d < PCA_EXP_FLOOR ? 0.0f : e;
}

// MODE 0: scores + softmax -> probs.  MODE 1: probs . b_fold -> out.
template <int DT, int MODE>
__global__ __launch_bounds__(PCA_NW * 64, 2) void pulid_tile_kernel(const PulidParams p) {
    using V8 = typename Half<DT>::V8;
    using HT = typename Half<DT>::T;
    constexpr int NT = PCA_NW * 64;
    __shared__ __attribute__((aligned(16))) uint8_t pca_lds[PCA_LDS];
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
    typedef __attribute__((address_space(3))) v4i lds_v4i;
    lds_u8 *const L8 = (lds_u8 *)pca_lds;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 31, h = lane >> 5;
    const int wr = wave & 1, wc = wave >> 1;
    const int group = blockIdx.x % p.groups;
    const long long row0 = (long long)(blockIdx.x / p.groups) * PCA_ROWS + wr * 32;
    const int col0 = group * PCA_COLS; // first column of D of this workgroup (a key, or an output channel)
    const int K = MODE == 0 ? p.C : p.J;
    const int N = p.N;
    const bool active = row0 < p.T; // (wave-uniform: an idle wave still stages and meets the barriers)
    const long long row = row0 + lr;
    const bool live = row < p.T;
    const uint16_t *brow = p.b + (size_t)(live ? row : p.T - 1) * p.ldb + 8 * h;

    // ---- the A pieces of one step, into registers ----
    // MODE 0: piece (kr, kc) = 8 channels k0 + 8 kc of key col0 + kr.  u = tid + NT i: 16 consecutive lanes read one key's 256 contiguous bytes.
    // MODE 1: unit (pc, cb) = the 8 keys k0 + 8 pc .. +7 x the 8 channels col0 + 8 cb .. +7: one 16-byte load per key, transposed at the write.
    v4i areg[8];
    auto load_a = [&](int k0) {
        if constexpr (MODE == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int u = tid + NT * i;
                const int kr = u >> 4, kc = u & 15;
                const int key = col0 + kr;
                areg[i] = v4i{0, 0, 0, 0};
                if ((key & 31) < N) areg[i] = *reinterpret_cast<const v4i *>(p.a + (size_t)key * p.C + k0 + kc * 8);
            }
        } else {
            const int cb = tid & 15, pc = tid >> 4;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int key = k0 + 8 * pc + i;
                areg[i] = v4i{0, 0, 0, 0};
                if ((key & 31) < N) areg[i] = *reinterpret_cast<const v4i *>(p.a + (size_t)key * p.C + col0 + cb * 8);
            }
        }
    };
    auto store_a = [&]() {
        if constexpr (MODE == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int u = tid + NT * i;
                const int kr = u >> 4, kc = u & 15;
                *(lds_v4i *)(L8 + (kr * 256 + ((kc ^ (kr & 15)) << 4))) = areg[i];
            }
        } else {
            const int cb = tid & 15, pc = tid >> 4;
#pragma unroll
            for (int e = 0; e < 8; e++) { // channel row 8 cb + e: the e-th 16-bit value of every key row, keys in natural order
                const v4i col = transpose8x8_piece(areg, e);
                const int cr = 8 * cb + e;
                *(lds_v4i *)(L8 + (cr * 256 + ((pc ^ (cr & 15)) << 4))) = col;
            }
        }
    };
    V8 bnext[8];
    auto load_b = [&](int k0) {
#pragma unroll
        for (int ds = 0; ds < 8; ds++) bnext[ds] = *reinterpret_cast<const V8 *>(brow + k0 + 16 * ds);
    };

    // fragment read offsets: accumulator tile at of this wave = columns col0 + 64 wc + 32 at + lr
    unsigned ka[8];
#pragma unroll
    for (int ds = 0; ds < 8; ds++) ka[ds] = (64 * wc + lr) * 256 + (((2 * ds + h) ^ (lr & 15)) << 4);

    v16f acc[2];
#pragma unroll
    for (int at = 0; at < 2; at++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[at][r] = 0.f;

    load_a(0);
    load_b(0);
    for (int k0 = 0; k0 < K; k0 += PCA_KSTEP) {
        __syncthreads(); // the previous step's reads are done
        store_a();
        V8 bf[8];
#pragma unroll
        for (int ds = 0; ds < 8; ds++) bf[ds] = bnext[ds];
        __syncthreads();
        if (k0 + PCA_KSTEP < K) { // in flight while the MFMAs run
            load_a(k0 + PCA_KSTEP);
            load_b(k0 + PCA_KSTEP);
        }
        if (active) {
#pragma unroll
            for (int ds = 0; ds < 8; ds++)
#pragma unroll
                for (int at = 0; at < 2; at++) {
                    const v4i aw = *(const lds_v4i *)(L8 + (ka[ds] + at * 8192));
                    acc[at] = Half<DT>::mfma32(__builtin_bit_cast(V8, aw), bf[ds], acc[at]);
                }
        }
    }
    if (!live) return; // (no barrier below)

    if constexpr (MODE == 0) {
        const float mean = p.stats[2 * row], rstd = p.stats[2 * row + 1];
#pragma unroll
        for (int at = 0; at < 2; at++) {
            const int key0 = col0 + 64 * wc + 32 * at; // the head's first key: lane (lr, h) holds the keys key0 + score_key(r, h)
            if (p.dbg) {
#pragma unroll
                for (int g = 0; g < 4; g++)
                    *reinterpret_cast<v4f *>(p.dbg + (size_t)row * p.J + key0 + 8 * g + 4 * h) =
                        v4f{acc[at][4 * g], acc[at][4 * g + 1], acc[at][4 * g + 2], acc[at][4 * g + 3]};
            }
            // s = rstd (acc - mean colsum) + cbias, one rounding per operation
            float s[16];
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const v4f cs = *reinterpret_cast<const v4f *>(p.colsum + key0 + 8 * g + 4 * h);
                const v4f cb = *reinterpret_cast<const v4f *>(p.cbias + key0 + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float mc = mean * cs[e];
                    const float d = acc[at][4 * g + e] - mc;
                    const float sd = rstd * d;
                    s[4 * g + e] = score_key(4 * g + e, h) < N ? sd + cb[e] : -INFINITY;
                }
            }
            // softmax over the head's 32 keys: the maximum (exact in any order), e = exp(s - m), the lane's 16 terms summed in register order, the
            // two halves added (a + b = b + a: both lanes hold the same sum), p = round16(e / sum)
            float m = s[0];
#pragma unroll
            for (int r = 1; r < 16; r++) m = fmaxf(m, s[r]);
            m = fmaxf(m, __shfl_xor(m, 32));
            float ex[16];
            float l = 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                ex[r] = pulid_exp(s[r] - m);
                l += ex[r];
            }
            l = l + __shfl_xor(l, 32);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const unsigned lo = pack2<DT>(ex[4 * g] / l, ex[4 * g + 1] / l);
                const unsigned hi = pack2<DT>(ex[4 * g + 2] / l, ex[4 * g + 3] / l);
                *reinterpret_cast<v2i *>(p.dst + (size_t)row * p.ldd + key0 + 8 * g + 4 * h) = v2i{(int)lo, (int)hi};
            }
        }
    } else {
        // out = round16(out_scale * round16(o)): both roundings explicit (ip_attention.hip's output rule; the empty asm statements keep the fp16
        // build from folding a product and the conversion behind it into one mixed-precision FMA)
#pragma unroll
        for (int at = 0; at < 2; at++) {
            const int c0 = col0 + 64 * wc + 32 * at;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                if (p.dbg)
                    *reinterpret_cast<v4f *>(p.dbg + (size_t)row * p.C + c0 + 8 * g + 4 * h) =
                        v4f{acc[at][4 * g], acc[at][4 * g + 1], acc[at][4 * g + 2], acc[at][4 * g + 3]};
                float t[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float v = acc[at][4 * g + e];
                    asm volatile("" : "+v"(v));
                    float u = round16<HT>(v) * p.out_scale;
                    asm volatile("" : "+v"(u));
                    t[e] = u;
                }
                *reinterpret_cast<v2i *>(p.dst + (size_t)row * p.ldd + c0 + 8 * g + 4 * h) =
                    v2i{(int)pack2<DT>(t[0], t[1]), (int)pack2<DT>(t[2], t[3])};
            }
        }
    }
}

template <int DT> static void launch_pulid(const PulidParams &ps, const PulidParams &po, long long row_tiles, hipStream_t st) {
    hipLaunchKernelGGL((pulid_tile_kernel<DT, 0>), dim3((unsigned)(row_tiles * ps.groups)), dim3(PCA_NW * 64), 0, st, ps);
    hipLaunchKernelGGL((pulid_tile_kernel<DT, 1>), dim3((unsigned)(row_tiles * po.groups)), dim3(PCA_NW * 64), 0, st, po);
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_pulid_ca(const svdq_pulid_ca_args *a, void *stream) {
    if (!a) { set_error("svdq_pulid_ca: args is NULL"); return SVDQ_E_INVALID; }
    if (!a->x || !a->stats || !a->a_fold || !a->colsum || !a->cbias || !a->b_fold || !a->probs || !a->out) {
        set_error("svdq_pulid_ca: x, stats, a_fold, colsum, cbias, b_fold, probs and out are required");
        return SVDQ_E_INVALID;
    }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("svdq_pulid_ca: unknown dtype %d", a->dtype); return SVDQ_E_INVALID; }
    if (a->T < 1 || a->C < 1 || a->H < 1) { set_error("svdq_pulid_ca: need T=%d, C=%d, H=%d >= 1", a->T, a->C, a->H); return SVDQ_E_INVALID; }
    if (a->N < 1) { set_error("svdq_pulid_ca: N=%d identity tokens per head: at least 1", a->N); return SVDQ_E_INVALID; }
    if (a->N > 32) { set_error("svdq_pulid_ca: N=%d identity tokens per head: at most 32 (a 32-key MFMA tile is one head)", a->N); return SVDQ_E_UNSUPPORTED; }
    if (a->C % 128) { set_error("svdq_pulid_ca: C=%d: only multiples of 128 are implemented", a->C); return SVDQ_E_UNSUPPORTED; }
    if (a->H % 4) { set_error("svdq_pulid_ca: H=%d: only multiples of 4 are implemented (a workgroup owns 128 keys)", a->H); return SVDQ_E_UNSUPPORTED; }
    if (a->H * 32 > 512) { set_error("svdq_pulid_ca: H=%d: H * 32 = %d keys, at most 512 are implemented", a->H, a->H * 32); return SVDQ_E_UNSUPPORTED; }
    if (a->ldx < a->C || a->ldo < a->C) {
        set_error("svdq_pulid_ca: row strides (ldx=%d ldo=%d) must be at least C = %d", a->ldx, a->ldo, a->C);
        return SVDQ_E_INVALID;
    }
    if (((uintptr_t)a->x | (uintptr_t)a->a_fold | (uintptr_t)a->b_fold | (uintptr_t)a->probs | (uintptr_t)a->out | (uintptr_t)a->colsum |
         (uintptr_t)a->cbias | (uintptr_t)a->acc | (uintptr_t)a->o_acc) & 15 || (uintptr_t)a->stats & 7 || (a->ldx | a->ldo) % 8) {
        set_error("svdq_pulid_ca: x, a_fold, b_fold, probs, out, colsum, cbias (and acc, o_acc) must be 16-byte aligned, stats 8-byte, the strides a multiple of 8");
        return SVDQ_E_INVALID;
    }
    if (!(a->out_scale - a->out_scale == 0.f)) { set_error("svdq_pulid_ca: out_scale must be finite"); return SVDQ_E_INVALID; }
    const int J = a->H * 32;
    const long long row_tiles = ((long long)a->T + PCA_ROWS - 1) / PCA_ROWS;
    if (row_tiles * (a->C / 128) > 0x7fffffffLL) { set_error("svdq_pulid_ca: T=%d x C=%d exceeds the grid", a->T, a->C); return SVDQ_E_INVALID; }
    PulidParams ps, po;
    ps.a = (const uint16_t *)a->a_fold; ps.b = (const uint16_t *)a->x; ps.stats = a->stats; ps.colsum = a->colsum; ps.cbias = a->cbias;
    ps.dst = (uint16_t *)a->probs; ps.dbg = a->acc; ps.ldb = a->ldx; ps.ldd = J;
    ps.T = a->T; ps.C = a->C; ps.J = J; ps.N = a->N; ps.groups = J / 128; ps.out_scale = a->out_scale;
    po = ps;
    po.a = (const uint16_t *)a->b_fold; po.b = (const uint16_t *)a->probs; po.dst = (uint16_t *)a->out; po.dbg = a->o_acc;
    po.ldb = J; po.ldd = a->ldo; po.groups = a->C / 128;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == SVDQ_BF16) launch_pulid<SVDQ_BF16>(ps, po, row_tiles, st);
    else launch_pulid<SVDQ_FP16>(ps, po, row_tiles, st);
    return hip_check(hipGetLastError(), "svdq_pulid_ca launch");
}
