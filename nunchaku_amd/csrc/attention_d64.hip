// svdq_attention_d64: the attention of Stable Diffusion XL's transformer blocks (reference: NunchakuSDXLFA2Processor,
// nunchaku/models/attention_processors/sdxl.py -> a chunk of the QKV projection, three view / transpose copies and torch's SDPA; here one
// launch that reads Q, K and V in place from what the projections wrote):
//
//   out[b, t, h, :] = round16( softmax_n(scale * q[b,t,h,:] . k[b,n,h,:]) . v[b,n,h,:] ),   head dim 64, n < N, no mask
//
// Shape of the problem: self-attention over 4096 (10 heads) or 1024 (20 heads) tokens and cross-attention over 77 text keys, batch 2 under
// classifier-free guidance.  4096 keys of one head are 1 MiB of K and V, so nothing is resident (cross_attention.hip keeps <= 320 keys in
// LDS): a workgroup (4 waves) owns a 128-row query tile of one (sample, head) and STREAMS K and V through LDS in 64-key chunks, double
// buffered: 2 x (8 KiB K + 8 KiB V^T) = 32 KiB.  Per chunk: the loads of chunk c + 1 are issued into registers, chunk c is computed from
// buffer c & 1, the registers are written to buffer (c + 1) & 1 (last read in iteration c - 1, which every wave left through the previous
// barrier), one barrier.
//
// Fragments and arithmetic are attn_frag.h's, as in cross_attention.hip, at D = 64 (S^T = K Q^T, O^T = V^T P^T on the 32x32x16 MFMA, a lane
// owning a query row; four K-steps of Q stay in registers for the whole walk; online softmax over chunks of 64 keys from key 0: exp2 with
// scale * log2(e); attn_frag.h states the softmax contract).
// LDS images: a K row and a V^T row are both 128 bytes = 8 pieces of 16 bytes; two rows cover the 64 banks once, so piece p of row r lives at
// column p ^ ((r >> 1) & 7): the sixteen rows of a ds_read_b128 lane group fall on sixteen distinct 16-byte slots.
// V is transposed on its way to LDS: a thread loads 2 channels (one dword) of 8 keys, in the key order the S accumulator delivers
// (piece j = keys 16 (j / 2) + 4 (j % 2) + {0..3, 8..11}), and writes one piece per channel: P^T goes from the S accumulator to the PV MFMA
// without a cross-lane exchange.
// Keys at or beyond N (only the last chunk holds any) are never loaded: their K and V images are zeros (0 x NaN is NaN in the matrix unit)
// and their scores -inf, probability exactly 0.  Rows at or beyond T: loads clamped to row T - 1, stores skipped.  Every offset is formed
// in 64 bits.  No atomics, no workspace; every output element is produced by one lane in a fixed order: two launches are bit-equal.
#include "svdq_common.h"
#include "attn_frag.h"

namespace svdq {

struct AttnD64Params {
    const uint16_t *q, *k, *v;
    uint16_t *out;
    long long q_bs, k_bs, v_bs, out_bs; // batch strides in elements (0 at B = 1)
    int ldq, ldk, ldv, ldo;             // row strides in elements
    int T, H, N;
    float c;                            // exponent factor: scale * log2(e)
};

constexpr int AD_NW = 4;            // waves per workgroup
constexpr int AD_ROWS = AD_NW * 32; // query rows per tile
constexpr int AD_CHUNK = 64;        // keys per online-softmax step and per LDS stage
constexpr int AD_D = 64;
constexpr int AD_STAGE = 2 * AD_CHUNK * AD_D * 2; // bytes of one stage: K [64 keys][128 B], then V^T [64 channels][128 B]

template <int DT>
__global__ __launch_bounds__(AD_NW * 64) void attention_d64_kernel(const AttnD64Params p) {
    using V8 = typename Half<DT>::V8;
    constexpr int D = AD_D, KS = D / 16, NDT = D / 32, RB = 128; // RB: bytes of a K row and of a V^T row in LDS
    constexpr unsigned VBASE = AD_CHUNK * RB;
    __shared__ __attribute__((aligned(16))) uint8_t ad_lds[2 * AD_STAGE];
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
    typedef __attribute__((address_space(3))) v4i lds_v4i;
    lds_u8 *const L8 = (lds_u8 *)ad_lds;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 31, h = lane >> 5;
    const int b = blockIdx.y / p.H, head = blockIdx.y % p.H;
    const int N = p.N;
    const int nch = (N + AD_CHUNK - 1) / AD_CHUNK;

    const uint16_t *kh = p.k + (size_t)b * (size_t)p.k_bs + (size_t)head * D;
    const uint16_t *vh = p.v + (size_t)b * (size_t)p.v_bs + (size_t)head * D;

    // ---- staging roles (loop invariants).  K: two 16-byte pieces per thread, piece kc of key kr0 and of key kr0 + 32.
    //      V: channels 2 cp, 2 cp + 1 of the 8 keys of piece vj ----
    const int kr0 = tid >> 3, kc = tid & 7;
    const unsigned kw0 = kr0 * RB + ((kc ^ ((kr0 >> 1) & 7)) << 4);
    const unsigned kw1 = kw0 + 32 * RB; // ((kr0 + 32) >> 1) & 7 == (kr0 >> 1) & 7
    const int cp = tid & 31, vj = tid >> 5;
    const int vkey0 = 16 * (vj >> 1) + 4 * (vj & 1);
    const unsigned vw = VBASE + 2 * cp * RB + ((vj ^ (cp & 7)) << 4); // rows 2 cp and 2 cp + 1 share (row >> 1) & 7 == cp & 7

    v4i kreg[2];
    unsigned vreg[8];
    auto load_chunk = [&](int ch) {
        const int key0 = ch * AD_CHUNK;
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
    };
    auto store_chunk = [&](int buf) {
        const unsigned base = buf * AD_STAGE;
        *(lds_v4i *)(L8 + (base + kw0)) = kreg[0];
        *(lds_v4i *)(L8 + (base + kw1)) = kreg[1];
        v4i lo, hi; // channel 2 cp: the low halves of the 8 keys; channel 2 cp + 1: the high halves
        transpose8x2_pieces(vreg, lo, hi);
        *(lds_v4i *)(L8 + (base + vw)) = lo;
        *(lds_v4i *)(L8 + (base + vw + RB)) = hi;
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

    const int q0 = blockIdx.x * AD_ROWS + wave * 32;
    const bool active = q0 < p.T; // (wave-uniform: an inactive wave still stages and passes every barrier)
    const int row = q0 + lr;
    const bool live = row < p.T;
    V8 qf[KS];
    {
        const uint16_t *qrow = p.q + (size_t)b * (size_t)p.q_bs + (size_t)(live ? row : p.T - 1) * p.ldq + (size_t)head * D + 8 * h;
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
        if (active) {
            const unsigned base = (ch & 1) * AD_STAGE;
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
            // ---- keys at or beyond N (only the last chunk can hold any) ----
            if (N < (ch + 1) * AD_CHUNK) {
#pragma unroll
                for (int kt = 0; kt < 2; kt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) s[kt][r] = AD_CHUNK * ch + 32 * kt + score_key(r, h) < N ? s[kt][r] : -INFINITY;
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
    // ---- round16(o / l): 16-byte stores ----
    const float inv = 1.0f / l;
    uint16_t *orow = p.out + (size_t)b * (size_t)p.out_bs + (size_t)(live ? row : p.T - 1) * p.ldo + (size_t)head * D + 8 * h;
#pragma unroll
    for (int dt = 0; dt < NDT; dt++)
#pragma unroll
        for (int j2 = 0; j2 < 2; j2++) {
            const v4i w = o_tile_piece<DT>(o[dt], j2, inv);
            if (live) *reinterpret_cast<v4i *>(orow + 32 * dt + 16 * j2) = w;
        }
}

// the bytes [lo, hi) an operand of `rows` rows spans
static void ad_extent(const void *ptr, int B, long long bs, int rows, int ld, long long width, uintptr_t *lo, uintptr_t *hi) {
    const long long elems = (B > 1 ? (long long)(B - 1) * bs : 0) + (long long)(rows - 1) * ld + width;
    *lo = (uintptr_t)ptr;
    *hi = (uintptr_t)ptr + (uintptr_t)elems * 2;
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_attention_d64(const svdq_attention_d64_args *a, void *stream) {
    if (!a) { set_error("svdq_attention_d64: args is NULL"); return SVDQ_E_INVALID; }
    if (!a->q || !a->k || !a->v || !a->out) { set_error("svdq_attention_d64: q, k, v and out are required"); return SVDQ_E_INVALID; }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("svdq_attention_d64: unknown dtype %d", a->dtype); return SVDQ_E_INVALID; }
    if (a->head_dim != AD_D) { set_error("svdq_attention_d64: head_dim=%d: 64 is implemented", a->head_dim); return SVDQ_E_UNSUPPORTED; }
    if (a->B < 1 || a->T < 1 || a->H < 1 || a->N < 1) {
        set_error("svdq_attention_d64: need B=%d, T=%d, H=%d, N=%d >= 1", a->B, a->T, a->H, a->N);
        return SVDQ_E_INVALID;
    }
    if ((long long)a->B * a->H > 65535 || a->T > (1 << 30) || a->N > (1 << 30)) {
        set_error("svdq_attention_d64: B * H = %lld, T = %d, N = %d exceed the grid (65535, 2^30, 2^30)", (long long)a->B * a->H, a->T, a->N);
        return SVDQ_E_INVALID;
    }
    const long long row = (long long)a->H * AD_D;
    if (a->ldq < row || a->ldk < row || a->ldv < row || a->ldo < row) {
        set_error("svdq_attention_d64: row strides (ldq=%d ldk=%d ldv=%d ldo=%d) must be at least H * 64 = %lld", a->ldq, a->ldk, a->ldv, a->ldo, row);
        return SVDQ_E_INVALID;
    }
    if (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->out) & 15 || (a->ldq | a->ldk | a->ldv | a->ldo) % 8) {
        set_error("svdq_attention_d64: q, k, v and out rows must be 16-byte aligned (pointers, and strides a multiple of 8)");
        return SVDQ_E_INVALID;
    }
    if (a->B > 1) {
        const long long need_q = (long long)(a->T - 1) * a->ldq + row, need_k = (long long)(a->N - 1) * a->ldk + row;
        const long long need_v = (long long)(a->N - 1) * a->ldv + row, need_o = (long long)(a->T - 1) * a->ldo + row;
        if (a->q_bs < need_q || a->k_bs < need_k || a->v_bs < need_v || a->out_bs < need_o) {
            set_error("svdq_attention_d64: batch strides (q_bs=%lld k_bs=%lld v_bs=%lld out_bs=%lld) must be at least (rows - 1) * ld + H * 64 = "
                      "%lld, %lld, %lld, %lld", (long long)a->q_bs, (long long)a->k_bs, (long long)a->v_bs, (long long)a->out_bs, need_q, need_k, need_v, need_o);
            return SVDQ_E_INVALID;
        }
        if ((a->q_bs | a->k_bs | a->v_bs | a->out_bs) % 8) {
            set_error("svdq_attention_d64: batch strides (q_bs=%lld k_bs=%lld v_bs=%lld out_bs=%lld) must be a multiple of 8: every sample 16-byte aligned",
                      (long long)a->q_bs, (long long)a->k_bs, (long long)a->v_bs, (long long)a->out_bs);
            return SVDQ_E_INVALID;
        }
    }
    {
        uintptr_t olo, ohi, lo, hi;
        ad_extent(a->out, a->B, a->out_bs, a->T, a->ldo, row, &olo, &ohi);
        const void *in[3] = {a->q, a->k, a->v};
        const long long bs[3] = {a->q_bs, a->k_bs, a->v_bs};
        const int rows[3] = {a->T, a->N, a->N}, ld[3] = {a->ldq, a->ldk, a->ldv};
        const char *names[3] = {"q", "k", "v"};
        for (int i = 0; i < 3; i++) {
            ad_extent(in[i], a->B, bs[i], rows[i], ld[i], row, &lo, &hi);
            if (lo < ohi && olo < hi) { set_error("svdq_attention_d64: out overlaps %s", names[i]); return SVDQ_E_INVALID; }
        }
    }
    if (!(a->scale > 0.f) || !(a->scale < INFINITY)) { set_error("svdq_attention_d64: scale must be positive and finite"); return SVDQ_E_INVALID; }
    AttnD64Params p;
    p.q = (const uint16_t *)a->q; p.k = (const uint16_t *)a->k; p.v = (const uint16_t *)a->v; p.out = (uint16_t *)a->out;
    const bool batched = a->B > 1;
    p.q_bs = batched ? a->q_bs : 0; p.k_bs = batched ? a->k_bs : 0; p.v_bs = batched ? a->v_bs : 0; p.out_bs = batched ? a->out_bs : 0;
    p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo;
    p.T = a->T; p.H = a->H; p.N = a->N;
    p.c = a->scale * 1.4426950408889634f;
    const dim3 grid((a->T + AD_ROWS - 1) / AD_ROWS, a->B * a->H);
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == SVDQ_BF16) hipLaunchKernelGGL((attention_d64_kernel<SVDQ_BF16>), grid, dim3(AD_NW * 64), 0, st, p);
    else hipLaunchKernelGGL((attention_d64_kernel<SVDQ_FP16>), grid, dim3(AD_NW * 64), 0, st, p);
    return hip_check(hipGetLastError(), "svdq_attention_d64 launch");
}
