// svdq_ip_attention: the image-prompt cross-attention of IP-Adapter (reference: nunchaku/models/ip_adapter/utils.py:346-372 -- a
// contiguous copy of Q, three view-transposes, SDPA, a transpose-reshape copy and a scaled add; here one launch that reads Q in place from
// the packed QKV buffer and K / V as the nn.Linear projections wrote them):
//
//   out[t, h, :] = round16( out_scale * round16( softmax_n(scale * q[t,h,:] . k[n,h,:]) . v[n,h,:] ) ),   1 <= N <= 256, head dim 128
//
// Shape of the problem: a few thousand queries against at most 256 keys.  K and V of ONE head (N x 128 each, <= 64 KiB each) stay in LDS
// for the whole life of a workgroup; a workgroup (8 waves) belongs to one head and walks 256-row query tiles of it, a wave owning 32 rows.
// All scores of a row are live at once (NKT = ceil(N / 32) accumulator tiles of the 32x32x16 MFMA): plain max / exp2 / sum, no online
// softmax, no rescaling of O.  P is rounded to 16 bits before the PV MFMA and the row sum is taken over the ROUNDED probabilities, the
// normalisation follows the MFMA (the softmax contract stated in attn_frag.h, without the running state).
//
// Fragments (the S^T = K Q^T / O^T = V^T P^T formulation of attention.hip, whose operand layouts are the verified ones; the code that
// depends on them alone is in attn_frag.h, shared with cross_attention.hip and attention_d64.hip):
//   * S^T[key][q]: A = K rows from LDS (lane: key = 32 kt + lr, d = 16 ds + 8 h .. +7), B = Q from registers (lane: q = lr, same d).
//     The accumulator gives lane (lr, h) the scores of query lr for the keys  32 kt + 8 (r / 4) + 4 h + r % 4.
//   * O^T[d][q]: B = P^T straight from those accumulator registers: the 8 registers r0 .. r0+7 (r0 = 8 (ks & 1)) of tile kt = ks / 2 are the
//     keys 16 ks + {4h .. 4h+3, 8+4h .. 8+4h+3}.  The order of the K dimension inside an MFMA is free as long as A agrees, so V^T is staged
//     into LDS with exactly that key order inside every 16-key group: piece j = 2 ks + h of row d holds those 8 keys -- no cross-lane
//     exchange between the two MFMAs (attention.hip pays 8 v_permlane32_swap per 64 keys for it; its V^T comes from the GEMM epilogue in
//     natural order, ours is staged by this kernel and may take any order).
//   * staging: K is a straight 16-byte copy (XOR-swizzled pieces, conflict-free ds_read_b128).  V is transposed on the way: a thread loads
//     the 8 key rows of one piece (16 bytes = 8 channels each), transposes the 8x8 block in registers and writes 8 ds_write_b128, one per
//     channel row; consecutive lanes take consecutive pieces of the same rows (128 contiguous LDS bytes per 8 lanes).
//   * keys at or beyond N: K and V rows are zeros in LDS (never read from memory) and their scores are set to -inf: probability 0.
//   * rows at or beyond T: the loads are clamped to row T - 1, the stores are skipped.
// No atomics, no workspace; every output element is produced by one lane in a fixed order: two launches are bit-equal.
#include "svdq_common.h"
#include "attn_frag.h"

namespace svdq {

struct IpAttnParams {
    const uint16_t *q, *k, *v;
    uint16_t *out;
    int ldq, ldk, ldv, ldo; // row strides in elements
    int T, H, N;
    int tiles;              // 256-row query tiles per head
    float c;                // exponent factor: scale * log2(e), or 1 when Q arrives prescaled
    float out_scale;
};

constexpr int IPA_NW = 8;             // waves per workgroup
constexpr int IPA_ROWS = IPA_NW * 32; // query rows per tile

constexpr int ipa_pow2_pieces(int nkt) { return nkt <= 1 ? 4 : nkt <= 2 ? 8 : nkt <= 4 ? 16 : 32; } // 16-byte pieces per V^T row (a power of two)
constexpr int ipa_lds_bytes(int nkt) { return nkt * 32 * 256 + 128 * ipa_pow2_pieces(nkt) * 16; }

template <int DT, int NKT>
__global__ __launch_bounds__(IPA_NW * 64, NKT <= 4 ? 4 : 2) void ip_attention_kernel(const IpAttnParams p) {
    using V8 = typename Half<DT>::V8;
    constexpr int NT = IPA_NW * 64;
    constexpr int KBYTES = NKT * 32 * 256;    // K: [NKT * 32 keys][256 B]
    constexpr int PRN = NKT * 4;              // pieces of a V^T row that hold keys
    constexpr int PR = ipa_pow2_pieces(NKT);  // row stride of V^T in pieces
    constexpr int RB = PR * 16;
    constexpr int SW_SHIFT = PR >= 16 ? 0 : (PR == 8 ? 1 : 2);
    constexpr int SW_MASK = PR >= 16 ? 15 : PR - 1;
    extern __shared__ __attribute__((aligned(16))) uint8_t ipa_lds[];
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
    typedef __attribute__((address_space(3))) v4i lds_v4i;
    lds_u8 *const L8 = (lds_u8 *)ipa_lds;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const int N = p.N;

    // ---- K of this head: NKT * 512 pieces, straight copy; piece kc of key kr lives at column kc ^ (kr & 15) ----
    {
        const uint16_t *kh = p.k + (size_t)head * 128;
#pragma unroll
        for (int i = 0; i < NKT; i++) {
            const int u = tid + NT * i;
            const int kr = u >> 4, kc = u & 15;
            v4i val = {0, 0, 0, 0};
            if (kr < N) val = *reinterpret_cast<const v4i *>(kh + (size_t)kr * p.ldk + kc * 8);
            *(lds_v4i *)(L8 + (kr * 256 + ((kc ^ (kr & 15)) << 4))) = val;
        }
    }
    // ---- V of this head, transposed: unit (piece j, channel block cb) = keys 16 (j / 2) + 4 (j % 2) + {0..3, 8..11} x channels 8 cb .. +7 ----
    {
        const uint16_t *vh = p.v + (size_t)head * 128;
        for (int u = tid; u < PRN * 16; u += NT) {
            const int j = u % PRN, cb = u / PRN;
            const int key0 = 16 * (j >> 1) + 4 * (j & 1);
            v4i rows[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int key = key0 + (i & 3) + 8 * (i >> 2);
                rows[i] = v4i{0, 0, 0, 0};
                if (key < N) rows[i] = *reinterpret_cast<const v4i *>(vh + (size_t)key * p.ldv + cb * 8);
            }
#pragma unroll
            for (int e = 0; e < 8; e++) { // channel 8 cb + e: the e-th 16-bit value of every key row
                const v4i col = transpose8x8_piece(rows, e);
                const int d = 8 * cb + e;
                *(lds_v4i *)(L8 + (KBYTES + d * RB + ((j ^ ((d >> SW_SHIFT) & SW_MASK)) << 4))) = col;
            }
        }
    }
    __syncthreads(); // the only barrier: LDS is read-only from here on

    // fragment read offsets (loop invariants)
    unsigned ka[8];
#pragma unroll
    for (int ds = 0; ds < 8; ds++) ka[ds] = lr * 256 + (((2 * ds + h) ^ (lr & 15)) << 4);
    const unsigned vrow = KBYTES + lr * RB;           // + dt * 32 * RB
    const unsigned vsw = (lr >> SW_SHIFT) & SW_MASK;  // (32 dt does not reach the swizzle bits)

    const float c = p.c;
    for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const int q0 = tile * IPA_ROWS + wave * 32;
        if (q0 >= p.T) continue; // (wave-uniform; no barrier below)
        const int row = q0 + lr;
        const bool live = row < p.T;
        V8 qf[8];
        {
            const uint16_t *qrow = p.q + (size_t)(live ? row : p.T - 1) * p.ldq + (size_t)head * 128 + 8 * h;
#pragma unroll
            for (int ds = 0; ds < 8; ds++) qf[ds] = *reinterpret_cast<const V8 *>(qrow + 16 * ds);
        }
        // ---- S^T = K Q^T ----
        v16f s[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; kt++) {
#pragma unroll
            for (int r = 0; r < 16; r++) s[kt][r] = 0.f;
#pragma unroll
            for (int ds = 0; ds < 8; ds++) {
                const v4i kw = *(const lds_v4i *)(L8 + (ka[ds] + kt * 8192));
                s[kt] = Half<DT>::mfma32(__builtin_bit_cast(V8, kw), qf[ds], s[kt]);
            }
        }
        // ---- keys at or beyond N (only the last tile can hold any) ----
        if (N < NKT * 32) {
#pragma unroll
            for (int r = 0; r < 16; r++) s[NKT - 1][r] = 32 * (NKT - 1) + score_key(r, h) < N ? s[NKT - 1][r] : -INFINITY;
        }
        // ---- softmax in one pass: lane holds half of the scores of query row lr, lane ^ 32 the other half ----
        const float m = row_max<NKT>(s);
        const float nmc = -(m * c);
        V8 pf[2 * NKT];
        float l = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2 * NKT; ks++) {
            const int kt = ks >> 1, r0 = 8 * (ks & 1);
            unsigned w[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                w[i] = prob_pair<DT>(s[kt][r0 + 2 * i], s[kt][r0 + 2 * i + 1], c, nmc);
                l = add_rounded<DT>(l, w[i]);
            }
            pf[ks] = __builtin_bit_cast(V8, v4i{(int)w[0], (int)w[1], (int)w[2], (int)w[3]});
        }
        l += __shfl_xor(l, 32);
        // ---- O^T = V^T P^T ----
        v16f o[4];
#pragma unroll
        for (int dt = 0; dt < 4; dt++) {
#pragma unroll
            for (int r = 0; r < 16; r++) o[dt][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 2 * NKT; ks++) {
                const v4i vw = *(const lds_v4i *)(L8 + (vrow + dt * 32 * RB + (((2 * ks + h) ^ vsw) << 4)));
                o[dt] = Half<DT>::mfma32(__builtin_bit_cast(V8, vw), pf[ks], o[dt]);
            }
        }
        // ---- round16(out_scale * round16(o / l)): both products are formed in fp32 and then rounded (the reference multiplies a 16-bit tensor by
        //      a Python float: an fp32 product, rounded once); the empty asm statements keep the fp16 build from folding product and conversion
        //      into one mixed-precision FMA, which would round the exact product instead.  Lane (lr, h) holds channels 32 dt + 8 g + 4 h + e;
        //      a v_permlane32_swap per dword pair gives every lane 8 consecutive channels: 16-byte stores (attn_frag.h's o_tile_piece with the
        //      second rounding inside; its own copy: see there) ----
        const float inv = 1.0f / l;
        uint16_t *orow = p.out + (size_t)row * p.ldo + (size_t)head * 128 + 8 * h;
#pragma unroll
        for (int dt = 0; dt < 4; dt++)
#pragma unroll
            for (int j2 = 0; j2 < 2; j2++) {
                unsigned x[2], y[2];
#pragma unroll
                for (int d2 = 0; d2 < 2; d2++) {
                    float t[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        float v = o[dt][8 * j2 + 4 * (i >> 1) + 2 * d2 + (i & 1)] * inv;
                        asm volatile("" : "+v"(v));
                        float u = round16<typename Half<DT>::T>(v) * p.out_scale;
                        asm volatile("" : "+v"(u));
                        t[i] = u;
                    }
                    x[d2] = pack2<DT>(t[0], t[1]);
                    y[d2] = pack2<DT>(t[2], t[3]);
                    const auto sw = __builtin_amdgcn_permlane32_swap(x[d2], y[d2], false, false);
                    x[d2] = sw[0];
                    y[d2] = sw[1];
                }
                if (live) *reinterpret_cast<v4i *>(orow + 32 * dt + 16 * j2) = v4i{(int)x[0], (int)x[1], (int)y[0], (int)y[1]};
            }
    }
}

template <int DT, int NKT> static hipError_t launch_ip_nkt(const IpAttnParams &p, dim3 grid, hipStream_t st) {
    constexpr int bytes = ipa_lds_bytes(NKT);
    if (bytes > 64 * 1024) { // beyond the default limit of dynamic LDS: raised once per device and instantiation
        static std::atomic<unsigned long long> raised{0};
        const hipError_t e = raise_dynamic_lds(reinterpret_cast<const void *>(&ip_attention_kernel<DT, NKT>), bytes, raised);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((ip_attention_kernel<DT, NKT>), grid, dim3(IPA_NW * 64), bytes, st, p);
    return hipSuccess;
}

template <int DT> static hipError_t launch_ip(const IpAttnParams &p, int nkt, dim3 grid, hipStream_t st) {
    switch (nkt) {
    case 1: return launch_ip_nkt<DT, 1>(p, grid, st);
    case 2: return launch_ip_nkt<DT, 2>(p, grid, st);
    case 3: return launch_ip_nkt<DT, 3>(p, grid, st);
    case 4: return launch_ip_nkt<DT, 4>(p, grid, st);
    case 5: return launch_ip_nkt<DT, 5>(p, grid, st);
    case 6: return launch_ip_nkt<DT, 6>(p, grid, st);
    case 7: return launch_ip_nkt<DT, 7>(p, grid, st);
    default: return launch_ip_nkt<DT, 8>(p, grid, st);
    }
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_ip_attention(const svdq_ip_attention_args *a, void *stream) {
    if (!a) { set_error("svdq_ip_attention: args is NULL"); return SVDQ_E_INVALID; }
    if (!a->q || !a->k || !a->v || !a->out) { set_error("svdq_ip_attention: q, k, v and out are required"); return SVDQ_E_INVALID; }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("svdq_ip_attention: unknown dtype %d", a->dtype); return SVDQ_E_INVALID; }
    if (a->head_dim != 128) { set_error("svdq_ip_attention: head_dim=%d: only 128 is implemented", a->head_dim); return SVDQ_E_UNSUPPORTED; }
    if (a->T < 1 || a->H < 1 || a->N < 1) { set_error("svdq_ip_attention: need T=%d, H=%d, N=%d >= 1", a->T, a->H, a->N); return SVDQ_E_INVALID; }
    if (a->N > 256) { set_error("svdq_ip_attention: N=%d image-prompt keys: at most 256 (K and V of one head stay in LDS)", a->N); return SVDQ_E_UNSUPPORTED; }
    if (a->H > 65535) { set_error("svdq_ip_attention: H=%d exceeds the grid", a->H); return SVDQ_E_INVALID; }
    const long long row = (long long)a->H * 128;
    if (a->ldq < row || a->ldk < row || a->ldv < row || a->ldo < row) {
        set_error("svdq_ip_attention: row strides (ldq=%d ldk=%d ldv=%d ldo=%d) must be at least H * 128 = %lld", a->ldq, a->ldk, a->ldv, a->ldo, row);
        return SVDQ_E_INVALID;
    }
    if (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->out) & 15 || (a->ldq | a->ldk | a->ldv | a->ldo) % 8) {
        set_error("svdq_ip_attention: q, k, v and out rows must be 16-byte aligned (pointers, and strides a multiple of 8)");
        return SVDQ_E_INVALID;
    }
    if ((!a->q_prescaled && (!(a->scale > 0.f) || !(a->scale < INFINITY))) || a->out_scale != a->out_scale) {
        set_error("svdq_ip_attention: scale must be positive and finite, out_scale a number");
        return SVDQ_E_INVALID;
    }
    IpAttnParams p;
    p.q = (const uint16_t *)a->q; p.k = (const uint16_t *)a->k; p.v = (const uint16_t *)a->v; p.out = (uint16_t *)a->out;
    p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo;
    p.T = a->T; p.H = a->H; p.N = a->N;
    p.tiles = (a->T + IPA_ROWS - 1) / IPA_ROWS;
    p.c = a->q_prescaled ? 1.0f : a->scale * 1.4426950408889634f;
    p.out_scale = a->out_scale;
    const int nkt = (a->N + 31) / 32;
    // workgroups per head: what the chip holds at once (256 CUs; two workgroups per CU while K and V take at most half the LDS), then the fewest that
    // need the same number of rounds -- every workgroup stages its head's K and V once, however many tiles it walks
    const int slots = 256 * (ipa_lds_bytes(nkt) * 2 <= 160 * 1024 ? 2 : 1);
    int per_head = slots / a->H;
    if (per_head < 1) per_head = 1;
    if (per_head > p.tiles) per_head = p.tiles;
    const int rounds = (p.tiles + per_head - 1) / per_head;
    per_head = (p.tiles + rounds - 1) / rounds;
    dim3 grid(per_head, a->H);
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = a->dtype == SVDQ_BF16 ? launch_ip<SVDQ_BF16>(p, nkt, grid, st) : launch_ip<SVDQ_FP16>(p, nkt, grid, st);
    if (e != hipSuccess) return hip_check(e, "svdq_ip_attention: raising the dynamic LDS limit");
    return hip_check(hipGetLastError(), "svdq_ip_attention launch");
}
