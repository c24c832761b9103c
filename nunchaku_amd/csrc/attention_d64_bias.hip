// svdq_attention_d64_bias: attention at head dimension 64 with an additive score bias that depends on (key - query) only, plus an optional
// per-key additive bias -- the self-attention of the T5 encoder (reference: transformers' T5Attention -> three view / transpose copies, a
// [B, H, T, N] score matmul rounded to 16 bits, the add of the [1, H, T, N] position bias, the add of the mask, a softmax, a second matmul and
// a copy back; here one launch on the projections' outputs in place, and no [H, T, N] tensor anywhere):
//
//   out[b, t, h, :] = round16( softmax_n(scale * q[b,t,h,:] . k[b,n,h,:] + rel_bias[h, n - t + T - 1] + key_bias[b, n]) . v[b,n,h,:] )
//
// Geometry, fragments and softmax are attention_d64.hip's (read its header first): a workgroup of 4 waves owns a 128-row query tile of one
// (sample, head), K and V^T stream through LDS in double-buffered 64-key chunks, S^T = K Q^T and O^T = V^T P^T on the 32x32x16 MFMA, a lane
// owning a query row, attn_frag.h's arithmetic and contract.  What is new is how the bias reaches the score registers.
//
// The bias stage.  For the query tile at row i0 and the key chunk at key j0 the scores need rel_bias[h, (j - i) + T - 1] for
// j - i in [j0 - i0 - 127, j0 - i0 + 63]: a WINDOW of 191 consecutive floats of the head's row, whatever the tile.  It is staged with the
// chunk's 64 key_bias values behind the K and V^T images of the same double-buffered stage, which grows from 16 KiB to 17 KiB:
//   [ K 8 KiB | V^T 8 KiB | window: 191 floats, slot 191: the chunk's live flag | key bias: 64 floats ]
// Every one of the 256 threads already loads K and V, so each takes ONE float more: thread t < 191 window entry t, thread 192 + j key j
// (wave 3 exactly).  Window entries whose index leaves [0, T + N - 2] belong to rows >= T or keys >= N only: they are staged as 0 and no
// address is formed for them.  Both are multiplied by log2(e) on their way to LDS, so the exponent stays one exp2 per score:
//   t = fma(s, scale * log2(e), window[(j - j0) - (i - i0) + 127]) + keyb[j - j0]        all fp32; p = exp2(t - max t)
// Reads.  Lane (lr, h) of wave w owns row i - i0 = 32 w + lr and its score register r of tile kt holds key j - j0 = 32 kt + 8 (r >> 2) + 4 h
// + (r & 3): one address register  127 - 32 w - lr + 4 h  and 32 immediate offsets; a run of 4 registers is 4 consecutive floats.  Bank
// picture of one scalar read: the 32 lanes of a half-wave sit on 32 consecutive floats (descending), the other half-wave 4 floats higher:
// 36 distinct dwords on 36 distinct banks of 64, the 28 shared ones broadcast -- conflict-free.  (A 16-byte read would need the run's first
// float on a 16-byte boundary, which holds for one lane in four.)  The key bias of a run is one aligned 16-byte read that a whole half-wave
// shares (2 addresses per wave).
//
// Exclusion.  finfo(bf16).min * log2(e) overflows fp32, and (-inf) - (-inf) in the running maximum is NaN.  The contract instead: a key_bias
// value at or below -2^100 (-inf included; a NaN too) EXCLUDES its key: it is staged as -inf, the key's probability is exactly 0.  Keys at
// or beyond N are excluded the same way (their K and V images are zeros, as in attention_d64.hip).  The running maximum of a row that has
// seen no key yet is replaced by 0 in the exponents (exp2(-inf - 0) = 0, never inf - inf); a row all of whose keys are excluded ends with
// l = 0 and is written as zeros.  Wave 3 holds the chunk's 64 key biases at staging: one ballot gives the chunk's LIVE flag; a chunk without
// a live key is skipped by every wave (its K and V are loaded, never looked at: NaN there changes nothing).  In a chunk WITH a live key the
// excluded keys' K and V rows do enter the matrix unit with weight 0 and must be finite, like every operand.  rel_bias must be finite.
// Every offset is formed in 64 bits.  No atomics, no workspace; every output element is produced by one lane in a fixed order: two launches
// are bit-equal.
#include "svdq_common.h"
#include "attn_frag.h"

namespace svdq {

struct AttnD64BiasParams {
    const uint16_t *q, *k, *v;
    uint16_t *out;
    const float *rel_bias, *key_bias;   // [H, T + N - 1]; [B, N] or NULL
    long long q_bs, k_bs, v_bs, out_bs; // batch strides in elements (0 at B = 1)
    int ldq, ldk, ldv, ldo;             // row strides in elements
    int T, H, N;
    float c;                            // exponent factor: scale * log2(e)
};

constexpr int AB_NW = 4;            // waves per workgroup
constexpr int AB_ROWS = AB_NW * 32; // query rows per tile
constexpr int AB_CHUNK = 64;        // keys per online-softmax step and per LDS stage
constexpr int AB_D = 64;
constexpr int AB_KV = 2 * AB_CHUNK * AB_D * 2;       // bytes of K [64 keys][128 B], then V^T [64 channels][128 B]
constexpr int AB_WIN = AB_ROWS + AB_CHUNK;           // window slots: 191 entries and the live flag
constexpr int AB_STAGE = AB_KV + (AB_WIN + AB_CHUNK) * 4; // one stage: 17 KiB
constexpr float AB_LOG2E = 1.4426950408889634f;
constexpr float AB_EXCLUDE = -0x1p100f;              // a key_bias at or below this excludes the key

// (3 waves per SIMD, as attention_d64_kernel: left alone the allocator takes 192 VGPRs, two waves; held to three it takes 165 and spills nothing)
template <int DT>
__attribute__((amdgpu_waves_per_eu(3, 3))) __global__ __launch_bounds__(AB_NW * 64) void attention_d64_bias_kernel(const AttnD64BiasParams p) {
    using V8 = typename Half<DT>::V8;
    constexpr int D = AB_D, KS = D / 16, NDT = D / 32, RB = 128; // RB: bytes of a K row and of a V^T row in LDS
    constexpr unsigned VBASE = AB_CHUNK * RB;
    __shared__ __attribute__((aligned(16))) uint8_t ab_lds[2 * AB_STAGE];
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
    typedef __attribute__((address_space(3))) v4i lds_v4i;
    typedef __attribute__((address_space(3))) v4f lds_v4f;
    typedef __attribute__((address_space(3))) float lds_f32;
    lds_u8 *const L8 = (lds_u8 *)ab_lds;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 31, h = lane >> 5;
    const int b = blockIdx.y / p.H, head = blockIdx.y % p.H;
    const int N = p.N, T = p.T;
    const int nch = (N + AB_CHUNK - 1) / AB_CHUNK;
    const int i0 = blockIdx.x * AB_ROWS;

    const uint16_t *kh = p.k + (size_t)b * (size_t)p.k_bs + (size_t)head * D;
    const uint16_t *vh = p.v + (size_t)b * (size_t)p.v_bs + (size_t)head * D;
    const float *relh = p.rel_bias + (size_t)head * (size_t)((long long)T + N - 1);
    const float *keyb = p.key_bias ? p.key_bias + (size_t)b * (size_t)N : nullptr;

    // ---- staging roles (loop invariants).  K: two 16-byte pieces per thread, piece kc of key kr0 and of key kr0 + 32.
    //      V: channels 2 cp, 2 cp + 1 of the 8 keys of piece vj.  Bias: slot tid of [window | key bias] ----
    const int kr0 = tid >> 3, kc = tid & 7;
    const unsigned kw0 = kr0 * RB + ((kc ^ ((kr0 >> 1) & 7)) << 4);
    const unsigned kw1 = kw0 + 32 * RB; // ((kr0 + 32) >> 1) & 7 == (kr0 >> 1) & 7
    const int cp = tid & 31, vj = tid >> 5;
    const int vkey0 = 16 * (vj >> 1) + 4 * (vj & 1);
    const unsigned vw = VBASE + 2 * cp * RB + ((vj ^ (cp & 7)) << 4); // rows 2 cp and 2 cp + 1 share (row >> 1) & 7 == cp & 7
    const long long wrel = (long long)tid - i0 - (AB_ROWS - 1) + (T - 1); // window slot tid at chunk 0: index into the head's rel_bias row
    const long long nrel = (long long)T + N - 1;

    v4i kreg[2];
    unsigned vreg[8];
    float breg;
    auto load_chunk = [&](int ch) {
        const int key0 = ch * AB_CHUNK;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int key = key0 + kr0 + 32 * i;
            kreg[i] = v4i{0, 0, 0, 0};
            if (key < N) kreg[i] = *reinterpret_cast<const v4i *>(kh + (size_t)key * p.ldk + kc * 8);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int key = key0 + vkey0 + (i & 3) + 8 * (i >> 2);
            vreg[i] = 0u;
            if (key < N) vreg[i] = *reinterpret_cast<const unsigned *>(vh + (size_t)key * p.ldv + cp * 2);
        }
        // the bias slot, RAW: nothing waits for it here (its conversion is store_chunk's, behind the chunk's arithmetic, where K and V are
        // waited for anyway).  Window: 0 outside the head's row; key bias: -inf at or beyond N, 0 without a key_bias
        if (tid < AB_WIN) { // (slot 191 is the flag's: thread 191 stages nothing)
            const long long idx = wrel + key0;
            breg = 0.f;
            if (tid < AB_WIN - 1 && idx >= 0 && idx < nrel) breg = relh[idx];
        } else {
            const int key = key0 + (tid - AB_WIN);
            breg = key < N ? 0.f : -INFINITY;
            if (key < N && keyb) breg = keyb[key];
        }
    };
    auto store_chunk = [&](int buf) {
        const unsigned base = buf * AB_STAGE;
        *(lds_v4i *)(L8 + (base + kw0)) = kreg[0];
        *(lds_v4i *)(L8 + (base + kw1)) = kreg[1];
        v4i lo, hi; // channel 2 cp: the low halves of the 8 keys; channel 2 cp + 1: the high halves
        transpose8x2_pieces(vreg, lo, hi);
        *(lds_v4i *)(L8 + (base + vw)) = lo;
        *(lds_v4i *)(L8 + (base + vw + RB)) = hi;
        // exponent units; a key bias at or below AB_EXCLUDE (or NaN): -inf.  Wave 3 holds the 64 key biases: one ballot is the live flag
        const float bval = (tid >= AB_WIN && !(breg > AB_EXCLUDE)) ? -INFINITY : breg * AB_LOG2E;
        const bool blive = __builtin_amdgcn_ballot_w64(tid >= AB_WIN && bval > -INFINITY) != 0ull;
        if (tid != AB_WIN - 1) *(lds_f32 *)(L8 + (base + AB_KV + 4 * tid)) = bval;
        if (tid == AB_WIN) *(lds_f32 *)(L8 + (base + AB_KV + 4 * (AB_WIN - 1))) = blive ? 1.f : 0.f;
    };

    // ---- fragment read offsets (loop invariants): K row lr (+ 32 kt), V^T row 32 dt + lr ----
    unsigned ka[KS], va[KS];
    {
        const unsigned sw = (lr >> 1) & 7; // (32 kt + lr) >> 1 and (32 dt + lr) >> 1 have the same low three bits
#pragma unroll
        for (int ds = 0; ds < KS; ds++) {
            ka[ds] = lr * RB + (((2 * ds + h) ^ sw) << 4);
            va[ds] = VBASE + ka[ds];
        }
    }
    // bias read offsets: the window entry of (this lane's row, key 4 h of the chunk); the key bias of key 4 h
    const unsigned wa = AB_KV + 4 * (AB_ROWS - 1 - 32 * wave - lr + 4 * h);
    const unsigned ba = AB_KV + 4 * AB_WIN + 16 * h;

    const int q0 = i0 + wave * 32;
    const bool active = q0 < T; // (wave-uniform: an inactive wave still stages and passes every barrier)
    const int row = q0 + lr;
    const bool live = row < T;
    V8 qf[KS];
    {
        const uint16_t *qrow = p.q + (size_t)b * (size_t)p.q_bs + (size_t)(live ? row : T - 1) * p.ldq + (size_t)head * D + 8 * h;
#pragma unroll
        for (int ds = 0; ds < KS; ds++) qf[ds] = *reinterpret_cast<const V8 *>(qrow + 16 * ds);
    }
    v16f o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; dt++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[dt][r] = 0.f;
    float m_run = -INFINITY, l = 0.f;
    const float c = p.c;

    load_chunk(0);
    store_chunk(0);
    __syncthreads();

    for (int ch = 0; ch < nch; ch++) {
        const bool more = ch + 1 < nch; // (uniform over the workgroup)
        if (more) load_chunk(ch + 1);
        const unsigned base = (ch & 1) * AB_STAGE;
        // the chunk's live flag (one LDS address for the whole wave)
        const bool some = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, *(const lds_f32 *)(L8 + (base + AB_KV + 4 * (AB_WIN - 1))))) != 0;
        if (active && some) {
            // ---- S^T = K Q^T for the 64 keys of this chunk ----
            v16f s[2];
#pragma unroll
            for (int kt = 0; kt < 2; kt++) {
#pragma unroll
                for (int r = 0; r < 16; r++) s[kt][r] = 0.f;
#pragma unroll
                for (int ds = 0; ds < KS; ds++) {
                    const v4i kw = *(const lds_v4i *)(L8 + (base + ka[ds] + kt * 32 * RB));
                    s[kt] = Half<DT>::mfma32(__builtin_bit_cast(V8, kw), qf[ds], s[kt]);
                }
            }
            // ---- t = s c + window + key bias, in exponent units; excluded keys and keys at or beyond N: -inf ----
#pragma unroll
            for (int kt = 0; kt < 2; kt++)
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const v4f kb = *(const lds_v4f *)(L8 + (base + ba + 4 * (32 * kt + 8 * g)));
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float w = *(const lds_f32 *)(L8 + (base + wa + 4 * (32 * kt + 8 * g + e)));
                        s[kt][4 * g + e] = __builtin_fmaf(s[kt][4 * g + e], c, w) + kb[e];
                    }
                }
            // ---- online softmax: lane holds 32 of the 64 scores of query row lr, lane ^ 32 the others.  A row without a key so far keeps
            //      m_run = -inf; its exponents take 0 for the maximum: every probability 0, alpha 0 ----
            const float m_new = fmaxf(m_run, row_max<2>(s));
            const float m_ref = m_new == -INFINITY ? 0.f : m_new;
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_ref);
            const float nm = -m_ref;
            m_run = m_new;
            V8 pf[4];
            float lc = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                const int kt = ks >> 1, r0 = 8 * (ks & 1);
                unsigned w[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    w[i] = pack2<DT>(__builtin_amdgcn_exp2f(s[kt][r0 + 2 * i] + nm), __builtin_amdgcn_exp2f(s[kt][r0 + 2 * i + 1] + nm));
                    lc = add_rounded<DT>(lc, w[i]);
                }
                pf[ks] = __builtin_bit_cast(V8, v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]});
            }
            l = l * alpha + lc;
            // ---- O^T = alpha O^T + V^T P^T ----
#pragma unroll
            for (int dt = 0; dt < NDT; dt++) {
#pragma unroll
                for (int r = 0; r < 16; r++) o[dt][r] *= alpha; // (element by element: the vector form becomes eight v_pk_mul_f32)
#pragma unroll
                for (int ks = 0; ks < 4; ks++) {
                    const v4i vv = *(const lds_v4i *)(L8 + (base + va[ks] + dt * 32 * RB));
                    o[dt] = Half<DT>::mfma32(__builtin_bit_cast(V8, vv), pf[ks], o[dt]);
                }
            }
        }
        if (more) store_chunk((ch + 1) & 1);
        __syncthreads();
    }
    if (!active) return;
    l += __shfl_xor(l, 32);
    // ---- round16(o / l): 16-byte stores.  l = 0: no key took part, the row is zeros ----
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    uint16_t *orow = p.out + (size_t)b * (size_t)p.out_bs + (size_t)(live ? row : T - 1) * p.ldo + (size_t)head * D + 8 * h;
#pragma unroll
    for (int dt = 0; dt < NDT; dt++)
#pragma unroll
        for (int j2 = 0; j2 < 2; j2++) {
            const v4i w = o_tile_piece<DT>(o[dt], j2, inv);
            if (live) *reinterpret_cast<v4i *>(orow + 32 * dt + 16 * j2) = w;
        }
}

// the bytes [lo, hi) an operand of `rows` rows spans
static void ab_extent(const void *ptr, int B, long long bs, int rows, int ld, long long width, uintptr_t *lo, uintptr_t *hi) {
    const long long elems = (B > 1 ? (long long)(B - 1) * bs : 0) + (long long)(rows - 1) * ld + width;
    *lo = (uintptr_t)ptr;
    *hi = (uintptr_t)ptr + (uintptr_t)elems * 2;
}

} // namespace svdq

using namespace svdq;

#define AB_NAME "svdq_attention_d64_bias"

// (svdq_attention_d64's list, then what the two bias operands add)
extern "C" int svdq_attention_d64_bias(const svdq_attention_d64_bias_args *a, void *stream) {
    if (!a) { set_error(AB_NAME ": args is NULL"); return SVDQ_E_INVALID; }
    if (!a->q || !a->k || !a->v || !a->out) { set_error(AB_NAME ": q, k, v and out are required"); return SVDQ_E_INVALID; }
    if (!a->rel_bias) { set_error(AB_NAME ": rel_bias is required"); return SVDQ_E_INVALID; }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error(AB_NAME ": unknown dtype %d", a->dtype); return SVDQ_E_INVALID; }
    if (a->head_dim != AB_D) { set_error(AB_NAME ": head_dim=%d: 64 is implemented", a->head_dim); return SVDQ_E_UNSUPPORTED; }
    if (a->B < 1 || a->T < 1 || a->H < 1 || a->N < 1) {
        set_error(AB_NAME ": need B=%d, T=%d, H=%d, N=%d >= 1", a->B, a->T, a->H, a->N);
        return SVDQ_E_INVALID;
    }
    if ((long long)a->B * a->H > 65535 || a->T > (1 << 30) || a->N > (1 << 30)) {
        set_error(AB_NAME ": B * H = %lld, T = %d, N = %d exceed the grid (65535, 2^30, 2^30)", (long long)a->B * a->H, a->T, a->N);
        return SVDQ_E_INVALID;
    }
    if ((long long)a->T + a->N - 1 > (1ll << 31)) {
        set_error(AB_NAME ": T + N - 1 = %lld exceeds 2^31 (the length of a rel_bias row)", (long long)a->T + a->N - 1);
        return SVDQ_E_INVALID;
    }
    const long long row = (long long)a->H * AB_D;
    if (a->ldq < row || a->ldk < row || a->ldv < row || a->ldo < row) {
        set_error(AB_NAME ": row strides (ldq=%d ldk=%d ldv=%d ldo=%d) must be at least H * 64 = %lld", a->ldq, a->ldk, a->ldv, a->ldo, row);
        return SVDQ_E_INVALID;
    }
    if (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->out) & 15 || (a->ldq | a->ldk | a->ldv | a->ldo) % 8) {
        set_error(AB_NAME ": q, k, v and out rows must be 16-byte aligned (pointers, and strides a multiple of 8)");
        return SVDQ_E_INVALID;
    }
    if (((uintptr_t)a->rel_bias | (uintptr_t)a->key_bias) & 3) { set_error(AB_NAME ": rel_bias and key_bias must be 4-byte aligned"); return SVDQ_E_INVALID; }
    if (a->B > 1) {
        const long long need_q = (long long)(a->T - 1) * a->ldq + row, need_k = (long long)(a->N - 1) * a->ldk + row;
        const long long need_v = (long long)(a->N - 1) * a->ldv + row, need_o = (long long)(a->T - 1) * a->ldo + row;
        if (a->q_bs < need_q || a->k_bs < need_k || a->v_bs < need_v || a->out_bs < need_o) {
            set_error(AB_NAME ": batch strides (q_bs=%lld k_bs=%lld v_bs=%lld out_bs=%lld) must be at least (rows - 1) * ld + H * 64 = "
                      "%lld, %lld, %lld, %lld", (long long)a->q_bs, (long long)a->k_bs, (long long)a->v_bs, (long long)a->out_bs, need_q, need_k, need_v, need_o);
            return SVDQ_E_INVALID;
        }
        if ((a->q_bs | a->k_bs | a->v_bs | a->out_bs) % 8) {
            set_error(AB_NAME ": batch strides (q_bs=%lld k_bs=%lld v_bs=%lld out_bs=%lld) must be a multiple of 8: every sample 16-byte aligned",
                      (long long)a->q_bs, (long long)a->k_bs, (long long)a->v_bs, (long long)a->out_bs);
            return SVDQ_E_INVALID;
        }
    }
    {
        uintptr_t olo, ohi, lo, hi;
        ab_extent(a->out, a->B, a->out_bs, a->T, a->ldo, row, &olo, &ohi);
        const void *in[3] = {a->q, a->k, a->v};
        const long long bs[3] = {a->q_bs, a->k_bs, a->v_bs};
        const int rows[3] = {a->T, a->N, a->N}, ld[3] = {a->ldq, a->ldk, a->ldv};
        const char *names[3] = {"q", "k", "v"};
        for (int i = 0; i < 3; i++) {
            ab_extent(in[i], a->B, bs[i], rows[i], ld[i], row, &lo, &hi);
            if (lo < ohi && olo < hi) { set_error(AB_NAME ": out overlaps %s", names[i]); return SVDQ_E_INVALID; }
        }
        // the two fp32 operands: [H, T + N - 1] and [B, N], contiguous
        const uintptr_t rlo = (uintptr_t)a->rel_bias, rhi = rlo + (uintptr_t)a->H * (uintptr_t)((long long)a->T + a->N - 1) * 4;
        const uintptr_t klo = (uintptr_t)a->key_bias, khi = klo + (uintptr_t)a->B * (uintptr_t)a->N * 4;
        if (rlo < ohi && olo < rhi) { set_error(AB_NAME ": out overlaps rel_bias"); return SVDQ_E_INVALID; }
        if (a->key_bias && klo < ohi && olo < khi) { set_error(AB_NAME ": out overlaps key_bias"); return SVDQ_E_INVALID; }
    }
    if (!(a->scale > 0.f) || !(a->scale < INFINITY)) { set_error(AB_NAME ": scale must be positive and finite"); return SVDQ_E_INVALID; }
    AttnD64BiasParams p;
    p.q = (const uint16_t *)a->q; p.k = (const uint16_t *)a->k; p.v = (const uint16_t *)a->v; p.out = (uint16_t *)a->out;
    p.rel_bias = (const float *)a->rel_bias; p.key_bias = (const float *)a->key_bias;
    const bool batched = a->B > 1;
    p.q_bs = batched ? a->q_bs : 0; p.k_bs = batched ? a->k_bs : 0; p.v_bs = batched ? a->v_bs : 0; p.out_bs = batched ? a->out_bs : 0;
    p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo;
    p.T = a->T; p.H = a->H; p.N = a->N;
    p.c = a->scale * AB_LOG2E;
    const dim3 grid((a->T + AB_ROWS - 1) / AB_ROWS, a->B * a->H);
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == SVDQ_BF16) hipLaunchKernelGGL((attention_d64_bias_kernel<SVDQ_BF16>), grid, dim3(AB_NW * 64), 0, st, p);
    else hipLaunchKernelGGL((attention_d64_bias_kernel<SVDQ_FP16>), grid, dim3(AB_NW * 64), 0, st, p);
    return hip_check(hipGetLastError(), AB_NAME " launch");
}
