// svdq_cross_attention: SANA's text cross-attention (reference: MultiHeadCrossAttention, src/SanaModel.cpp:147-190 -> flash-attention's
// mha_varlen_fwd over per-sample key ranges; here one launch that reads Q in place from q_linear's output and K / V as the two column halves
// of what kv_linear wrote):
//
//   out[b, t, h, :] = round16( softmax_n(scale * q[b,t,h,:] . k[n,h,:]) . v[n,h,:] ),   n in [key_offsets[b], key_offsets[b] + key_counts[b])
//
// head dim D = 72, 112 or 128; at most XA_MAX_KEYS = 320 keys per sample; offsets and counts are read on the device (no host sync).
//
// Shape of the problem: thousands of queries per sample against at most a few hundred keys of that sample.  A workgroup (8 waves) belongs
// to one (sample, head): it stages that pair's K and V into LDS ONCE (RESIDENT, not streamed: see DESIGN 6m), passes the only barrier and
// walks 256-row query tiles, a wave owning 32 rows.  300 keys are ten 32-key accumulator tiles -- too many to keep every score of a row
// live as ip_attention.hip does -- so a wave walks the resident keys in CHUNKS of 64 with an online softmax (attn_frag.h states its
// contract).  Chunks start at the sample's first key: a row's arithmetic depends on its own sample's keys
// only, not on where they lie in the buffer or on what other samples hold.
//
// Fragments are attn_frag.h's, shared with ip_attention.hip (S^T = K Q^T, O^T = V^T P^T on the 32x32x16 MFMA; V transposed while staging in
// the key order the accumulator delivers, so P^T goes from the S accumulator to the PV MFMA without a cross-lane exchange).  What the head
// dimension changes:
//   * K-steps of QK^T: KS = ceil(D / 16) = 5 / 7 / 8.  D = 72 is four and a half: the 16-byte piece of channels 72..79 is ZERO in LDS (K) and
//     in registers (Q) -- neither is loaded: those columns belong to the next head (or lie beyond H * D), and 0 * Inf would be NaN.
//   * K rows in LDS are 2 KS pieces = 160 / 224 / 256 bytes.  160 and 224 bytes step 8 consecutive rows over 8 distinct 32-byte bank groups:
//     ds_read_b128 is conflict-free without a swizzle; 256-byte rows keep ip_attention.hip's XOR swizzle.
//   * O^T tiles: ceil(D / 32) = 3 / 4 / 4.  The lanes of the last tile whose channel is >= D read V^T row D - 1 again (any finite row would
//     do: MFMA output rows are independent) and their 16-byte stores are skipped: D is a multiple of 8, so a store is whole or absent.
//   * V^T rows are kcap * 2 bytes (kcap = the key capacity of this launch, a multiple of 64): a multiple of 128 bytes, so the piece index is
//     XORed with (d & 7), which stays inside the chunk's 8 pieces.
// Keys at or beyond the sample's count inside its last chunk: K and V are zeros in LDS (never read from memory), scores -inf.
// A sample without keys: its rows are written as zeros (flash-attention does the same).  Rows at or beyond T: loads clamped to row T - 1,
// stores skipped.  No atomics, no workspace; every output element is produced by one lane in a fixed order: two launches are bit-equal.
#include "svdq_common.h"
#include "attn_frag.h"

namespace svdq {

struct XAttnParams {
    const uint16_t *q, *k, *v;
    uint16_t *out;
    const int32_t *key_offsets, *key_counts;
    int ldq, ldk, ldv, ldo; // row strides in elements
    int T, H, Nrows, max_keys;
    int kcap;               // key capacity of the LDS image: a multiple of 64, >= min(max_keys, Nrows)
    int tiles;              // 256-row query tiles per (sample, head)
    float c;                // exponent factor: scale * log2(e)
};

constexpr int XA_NW = 8;            // waves per workgroup
constexpr int XA_ROWS = XA_NW * 32; // query rows per tile
constexpr int XA_CHUNK = 64;        // keys per online-softmax step
constexpr int XA_MAX_KEYS = 320;    // D = 128: 320 * (256 + 256) bytes = 160 KiB, the LDS of a CU

constexpr int xa_krow_bytes(int d) { return (d + 15) / 16 * 32; }
constexpr int xa_lds_bytes(int d, int kcap) { return kcap * (xa_krow_bytes(d) + 2 * d); }

template <int DT, int D>
__global__ __launch_bounds__(XA_NW * 64, 2) void cross_attention_kernel(const XAttnParams p) {
    using V8 = typename Half<DT>::V8;
    constexpr int NT = XA_NW * 64;
    constexpr int KS = (D + 15) / 16;  // K-steps of QK^T
    constexpr int KP = 2 * KS;         // 16-byte pieces of a K row in LDS
    constexpr int KRB = KP * 16;
    constexpr int CB = D / 8;          // 16-byte pieces of a K / V row in memory
    constexpr int NDT = (D + 31) / 32; // O^T tiles
    constexpr int KSW = D == 128 ? 15 : 0;
    static_assert(D % 8 == 0 && D <= 128, "head dim");
    extern __shared__ __attribute__((aligned(16))) uint8_t xa_lds[];
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
    typedef __attribute__((address_space(3))) v4i lds_v4i;
    lds_u8 *const L8 = (lds_u8 *)xa_lds;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 31, h = lane >> 5;
    const int b = blockIdx.y / p.H, head = blockIdx.y % p.H;

    // ---- the sample's key range, clamped: count to [0, max_keys], range to [0, Nrows) ----
    int off = p.key_offsets[b], n = p.key_counts[b];
    n = n < 0 ? 0 : n > p.max_keys ? p.max_keys : n;
    if (off < 0 || off >= p.Nrows) n = 0;
    else if (n > p.Nrows - off) n = p.Nrows - off;
    if (n > p.kcap) n = p.kcap; // (cannot happen: kcap >= min(max_keys, Nrows); keeps every LDS address inside the allocation regardless)

    const size_t qbase = (size_t)b * p.T;
    if (n == 0) { // no keys: zero rows
        for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
            const int q0 = tile * XA_ROWS + wave * 32;
            for (int r = 0; r < 32; r++) {
                const int row = q0 + r;
                if (row < p.T && lane < CB) *reinterpret_cast<v4i *>(p.out + (qbase + row) * p.ldo + (size_t)head * D + lane * 8) = v4i{0, 0, 0, 0};
            }
        }
        return;
    }
    const int nch = (n + XA_CHUNK - 1) / XA_CHUNK;
    const int RB = p.kcap * 2;              // bytes of a V^T row
    const unsigned VBASE = p.kcap * KRB;

    // ---- K of this (sample, head): nch * 64 rows of KP pieces, straight copy; piece kc of key kr lives at column kc ^ (kr & KSW) ----
    {
        const uint16_t *kh = p.k + (size_t)off * p.ldk + (size_t)head * D;
        for (int u = tid; u < nch * XA_CHUNK * KP; u += NT) {
            const int kr = u / KP, kc = u % KP;
            v4i val = {0, 0, 0, 0};
            if (kr < n && kc < CB) val = *reinterpret_cast<const v4i *>(kh + (size_t)kr * p.ldk + kc * 8);
            *(lds_v4i *)(L8 + (kr * KRB + ((kc ^ (kr & KSW)) << 4))) = val;
        }
    }
    // ---- V, transposed: unit (piece j, channel block cb) = keys 16 (j / 2) + 4 (j % 2) + {0..3, 8..11} x channels 8 cb .. +7 ----
    {
        const uint16_t *vh = p.v + (size_t)off * p.ldv + (size_t)head * D;
        const int PRN = nch * 8;
        for (int u = tid; u < PRN * CB; u += NT) {
            const int j = u % PRN, cb = u / PRN;
            const int key0 = 16 * (j >> 1) + 4 * (j & 1);
            v4i rows[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int key = key0 + (i & 3) + 8 * (i >> 2);
                rows[i] = v4i{0, 0, 0, 0};
                if (key < n) rows[i] = *reinterpret_cast<const v4i *>(vh + (size_t)key * p.ldv + cb * 8);
            }
#pragma unroll
            for (int e = 0; e < 8; e++) { // channel 8 cb + e: the e-th 16-bit value of every key row
                const v4i col = transpose8x8_piece(rows, e);
                const int d = 8 * cb + e;
                *(lds_v4i *)(L8 + (VBASE + d * RB + ((j ^ (d & 7)) << 4))) = col;
            }
        }
    }
    __syncthreads(); // the only barrier: LDS is read-only from here on

    // fragment read offsets (loop invariants)
    unsigned ka[KS];
#pragma unroll
    for (int ds = 0; ds < KS; ds++) ka[ds] = lr * KRB + (((2 * ds + h) ^ (lr & KSW)) << 4);
    unsigned va[NDT], vsw[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) {
        const int d = 32 * dt + lr < D ? 32 * dt + lr : D - 1;
        va[dt] = VBASE + d * RB;
        vsw[dt] = d & 7;
    }

    const float c = p.c;
    for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int q0 = tile * XA_ROWS + wave * 32;
        if (q0 >= p.T) continue; // (wave-uniform; no barrier below)
        const int row = q0 + lr;
        const bool live = row < p.T;
        V8 qf[KS];
        {
            const uint16_t *qrow = p.q + (qbase + (live ? row : p.T - 1)) * p.ldq + (size_t)head * D + 8 * h;
#pragma unroll
            for (int ds = 0; ds < KS; ds++) {
                if (16 * ds + 8 < D) qf[ds] = *reinterpret_cast<const V8 *>(qrow + 16 * ds);
                else { // the half K-step: channels 16 ds + 8 .. +15 do not exist
                    v4i z = {0, 0, 0, 0};
                    if (h == 0) z = *reinterpret_cast<const v4i *>(qrow + 16 * ds);
                    qf[ds] = __builtin_bit_cast(V8, z);
                }
            }
        }
        v16f o[NDT];
#pragma unroll
        for (int dt = 0; dt < NDT; dt++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[dt][r] = 0.f;
        float m_run = -INFINITY, l = 0.f;

        for (int ch = 0; ch < nch; ch++) {
            // ---- S^T = K Q^T for the 64 keys of this chunk ----
            v16f s[2];
#pragma unroll
            for (int kt = 0; kt < 2; kt++) {
#pragma unroll
                for (int r = 0; r < 16; r++) s[kt][r] = 0.f;
#pragma unroll
                for (int ds = 0; ds < KS; ds++) {
                    const v4i kw = *(const lds_v4i *)(L8 + (ka[ds] + (2 * ch + kt) * 32 * KRB));
                    s[kt] = Half<DT>::mfma32(__builtin_bit_cast(V8, kw), qf[ds], s[kt]);
                }
            }
            // ---- keys at or beyond the count (only the last chunk can hold any) ----
            if (n < (ch + 1) * XA_CHUNK) {
#pragma unroll
                for (int kt = 0; kt < 2; kt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) s[kt][r] = XA_CHUNK * ch + 32 * kt + score_key(r, h) < n ? s[kt][r] : -INFINITY;
            }
            // ---- online softmax: lane holds 32 of the 64 scores of query row lr, lane ^ 32 the others ----
            const SoftmaxScale sc = online_softmax_scale(m_run, row_max<2>(s), c);
            m_run = sc.m;
            V8 pf[4];
            float lc = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                const int kt = ks >> 1, r0 = 8 * (ks & 1);
                unsigned w[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    w[i] = prob_pair<DT>(s[kt][r0 + 2 * i], s[kt][r0 + 2 * i + 1], c, sc.nmc);
                    lc = add_rounded<DT>(lc, w[i]);
                }
                pf[ks] = __builtin_bit_cast(V8, v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]});
            }
            l = l * sc.alpha + lc;
            // ---- O^T = alpha O^T + V^T P^T ----
#pragma unroll
            for (int dt = 0; dt < NDT; dt++) {
                o[dt] = o[dt] * sc.alpha;
#pragma unroll
                for (int ks = 0; ks < 4; ks++) {
                    const v4i vw = *(const lds_v4i *)(L8 + (va[dt] + (((8 * ch + 2 * ks + h) ^ vsw[dt]) << 4)));
                    o[dt] = Half<DT>::mfma32(__builtin_bit_cast(V8, vw), pf[ks], o[dt]);
                }
            }
        }
        l += __shfl_xor(l, 32);
        // ---- round16(o / l): 16-byte stores, cut at D (beyond it lies the next head, which another workgroup owns) ----
        const float inv = 1.0f / l;
        uint16_t *orow = p.out + (qbase + row) * p.ldo + (size_t)head * D + 8 * h;
#pragma unroll
        for (int dt = 0; dt < NDT; dt++)
#pragma unroll
            for (int j2 = 0; j2 < 2; j2++) {
                if (32 * dt + 16 * j2 >= D) continue; // (compile time: no lane of this pair has a channel)
                const v4i w = o_tile_piece<DT>(o[dt], j2, inv);
                if (live && 32 * dt + 16 * j2 + 8 * h < D) *reinterpret_cast<v4i *>(orow + 32 * dt + 16 * j2) = w;
            }
    }
}

template <int DT, int D> static hipError_t launch_xa(const XAttnParams &p, dim3 grid, hipStream_t st) {
    const int bytes = xa_lds_bytes(D, p.kcap);
    if (bytes > 64 * 1024) { // beyond the default limit of dynamic LDS: raised once per device and instantiation, to what XA_MAX_KEYS needs
        static std::atomic<unsigned long long> raised{0};
        const hipError_t e = raise_dynamic_lds(reinterpret_cast<const void *>(&cross_attention_kernel<DT, D>), xa_lds_bytes(D, XA_MAX_KEYS), raised);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((cross_attention_kernel<DT, D>), grid, dim3(XA_NW * 64), bytes, st, p);
    return hipSuccess;
}

template <int DT> static hipError_t launch_xa_d(const XAttnParams &p, int d, dim3 grid, hipStream_t st) {
    switch (d) {
    case 72: return launch_xa<DT, 72>(p, grid, st);
    case 112: return launch_xa<DT, 112>(p, grid, st);
    default: return launch_xa<DT, 128>(p, grid, st);
    }
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_cross_attention(const svdq_cross_attention_args *a, void *stream) {
    if (!a) { set_error("svdq_cross_attention: args is NULL"); return SVDQ_E_INVALID; }
    if (!a->q || !a->k || !a->v || !a->out || !a->key_offsets || !a->key_counts) {
        set_error("svdq_cross_attention: q, k, v, out, key_offsets and key_counts are required");
        return SVDQ_E_INVALID;
    }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("svdq_cross_attention: unknown dtype %d", a->dtype); return SVDQ_E_INVALID; }
    if (a->head_dim != 72 && a->head_dim != 112 && a->head_dim != 128) {
        set_error("svdq_cross_attention: head_dim=%d: 72, 112 and 128 are implemented", a->head_dim);
        return SVDQ_E_UNSUPPORTED;
    }
    if (a->B < 1 || a->T < 1 || a->H < 1) { set_error("svdq_cross_attention: need B=%d, T=%d, H=%d >= 1", a->B, a->T, a->H); return SVDQ_E_INVALID; }
    if (a->max_keys < 0 || a->Nrows < 0) { set_error("svdq_cross_attention: need max_keys=%d, Nrows=%d >= 0", a->max_keys, a->Nrows); return SVDQ_E_INVALID; }
    if (a->max_keys > XA_MAX_KEYS) {
        set_error("svdq_cross_attention: max_keys=%d: at most %d keys per sample (K and V of one sample and head stay in LDS)", a->max_keys, XA_MAX_KEYS);
        return SVDQ_E_UNSUPPORTED;
    }
    if ((long long)a->B * a->H > 65535 || a->T > (1 << 30)) {
        set_error("svdq_cross_attention: B * H = %lld, T = %d exceed the grid (65535, 2^30)", (long long)a->B * a->H, a->T);
        return SVDQ_E_INVALID;
    }
    const int D = a->head_dim;
    const long long row = (long long)a->H * D;
    if (a->ldq < row || a->ldk < row || a->ldv < row || a->ldo < row) {
        set_error("svdq_cross_attention: row strides (ldq=%d ldk=%d ldv=%d ldo=%d) must be at least H * head_dim = %lld", a->ldq, a->ldk, a->ldv, a->ldo, row);
        return SVDQ_E_INVALID;
    }
    if (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->out) & 15 || (a->ldq | a->ldk | a->ldv | a->ldo) % 8) {
        set_error("svdq_cross_attention: q, k, v and out rows must be 16-byte aligned (pointers, and strides a multiple of 8)");
        return SVDQ_E_INVALID;
    }
    if (((uintptr_t)a->key_offsets | (uintptr_t)a->key_counts) & 3) { set_error("svdq_cross_attention: key_offsets and key_counts must be 4-byte aligned"); return SVDQ_E_INVALID; }
    if (!(a->scale > 0.f) || !(a->scale < INFINITY)) { set_error("svdq_cross_attention: scale must be positive and finite"); return SVDQ_E_INVALID; }
    XAttnParams p;
    p.q = (const uint16_t *)a->q; p.k = (const uint16_t *)a->k; p.v = (const uint16_t *)a->v; p.out = (uint16_t *)a->out;
    p.key_offsets = a->key_offsets; p.key_counts = a->key_counts;
    p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo;
    p.T = a->T; p.H = a->H; p.Nrows = a->Nrows; p.max_keys = a->max_keys;
    const int bound = a->max_keys < a->Nrows ? a->max_keys : a->Nrows;
    p.kcap = bound < 1 ? XA_CHUNK : (bound + XA_CHUNK - 1) / XA_CHUNK * XA_CHUNK;
    p.tiles = (a->T + XA_ROWS - 1) / XA_ROWS;
    p.c = a->scale * 1.4426950408889634f;
    // workgroups per (sample, head): what the chip holds at once -- 256 CUs with ONE workgroup each, whatever the LDS image takes: a workgroup is
    // 2 waves on every SIMD and the kernel needs 134 - 172 VGPRs, so a second workgroup (4 waves per SIMD: at most 128 VGPRs) never fits -- then the
    // fewest that need the same number of rounds: every workgroup stages its K and V once, however many tiles it walks
    const int slots = 256;
    int per_bh = slots / (a->B * a->H);
    if (per_bh < 1) per_bh = 1;
    if (per_bh > p.tiles) per_bh = p.tiles;
    const int rounds = (p.tiles + per_bh - 1) / per_bh;
    per_bh = (p.tiles + rounds - 1) / rounds;
    dim3 grid(per_bh, a->B * a->H);
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = a->dtype == SVDQ_BF16 ? launch_xa_d<SVDQ_BF16>(p, D, grid, st) : launch_xa_d<SVDQ_FP16>(p, D, grid, st);
    if (e != hipSuccess) return hip_check(e, "svdq_cross_attention: raising the dynamic LDS limit");
    return hip_check(hipGetLastError(), "svdq_cross_attention launch");
}
