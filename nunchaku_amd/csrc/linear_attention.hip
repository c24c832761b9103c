// svdq_linear_attention: SANA's ReLU linear attention (reference: src/SanaModel.cpp:25-106 -- there the K/V reduction is an epilogue of the
// QKV GEMM that adds into vk with fp32 atomics (epilogues.cuh:552-761) and a second kernel multiplies by Q; here the QKV GEMM runs its plain
// epilogue and these kernels read the packed buffer it wrote, in place).  Per batch element b and head h, head dimension 32:
//
//   vk[i][j]  = sum_t V[t][i] * relu(K[t][j])          i, j < 32      fp32
//   vk[32][j] = sum_t relu(K[t][j])
//   out[t][i] = round16( (sum_j relu(Q[t][j]) * vk[i][j]) / (sum_j relu(Q[t][j]) * vk[32][j] + eps) )
//
// Both phases move 128 bytes per (token, head) for 2 * 33 * 32 flops: they are bound by bytes, not by arithmetic, and the shape of the
// kernels follows from that -- whole 128-byte lines per token, 16 bytes per lane, enough workgroups to fill the chip at B = 1, H = 36.
//
//   1. la_reduce_kernel, grid (chunks of 256 tokens, H, B), 4 waves: a wave stages its 64 token rows [K 32 | V 32] in LDS (relu applied to
//      the K half on the way: a bit operation on the 16-bit values) and runs 4 v_mfma_f32_32x32x16 steps with the TOKEN axis as the MFMA's K
//      dimension: A = V^T (lane (lr, h): channel lr, tokens 16 s + 8 h .. +7), B = relu(K) (same lanes, same tokens), so the accumulator
//      gives lane (lr, h) vk[8 (r / 4) + 4 h + r % 4][lr].  The operands are token-major in memory; the transpose is the LDS read (eight
//      16-bit reads per operand -- at one MFMA per 2 KiB of input nothing is gained by a faster one).  Row 32 is a second MFMA with A = ones.
//      The four waves' tiles are added in wave order and the chunk's [33, 32] fp32 partial goes to the workspace.  Tokens at or beyond T are
//      never read: their LDS rows are zeros.
//   2. la_finish_kernel: one thread per element of [B, H, 33, 32] adds the chunks' partials in chunk order; the sums go to the workspace
//      (what phase 3 reads) and to the caller's vk.
//   3. la_apply_kernel, grid (tiles of 128 tokens, pairs of heads, B), 256 threads = 128 tokens x 2 heads: the Q rows of the pair (128
//      contiguous bytes per token) are staged in LDS, vk of both heads is staged TRANSPOSED ([j][i], rows of 36 floats) so that a thread walks
//      j with packed fp32 FMAs over pairs of i; vk stays fp32 from the MFMA accumulator to the quotient.  The results replace the thread's
//      own Q row in LDS and leave as whole lines.
//
// No atomics: every partial and every sum is produced by one thread in a fixed order, two launches are bit-equal.  At most three launches
// (two when only vk is asked for), no allocation, no synchronisation.
#include "svdq_common.h"
#include "attn_frag.h"

namespace svdq {

constexpr int LA_VK = 33 * 32;   // floats of one [33, 32] tile
constexpr int LA_CHUNK = 256;    // tokens per reduce workgroup: 4 waves x 64
constexpr int LA_TILE = 128;     // tokens per apply workgroup
constexpr int LA_QROW = 144;     // bytes of a token row of the apply tile: 2 heads x 64 + 16 of padding
constexpr int LA_VKROW = 36;     // floats of a j row of the transposed vk image: i = 0..32, 3 of padding

struct LaParams {
    const uint16_t *q, *kv;
    uint16_t *out;
    float *vk;        // caller's [B, H, 33, 32] or NULL
    float *partials;  // workspace: [B, H, nchunks, 33, 32]
    float *sums;      // workspace: [B, H, 33, 32]
    long long q_bs, kv_bs, out_bs; // batch strides in elements
    int ldq, ldkv, ldo;            // row strides in elements
    int T, H, nchunks;
    float eps;
};

// relu of the two 16-bit floats of a dword (either format): a value with its sign bit set becomes +0
__device__ __forceinline__ int la_relu2(int x) {
    const unsigned m = ((unsigned)x >> 15) & 0x00010001u;
    return x & ~(int)((m << 16) - m);
}

template <int DT>
__global__ __launch_bounds__(256) void la_reduce_kernel(const LaParams p) {
    using V8 = typename Half<DT>::V8;
    __shared__ __attribute__((aligned(16))) uint16_t tile[4][64][64]; // [wave][token][K 32 | V 32]
    __shared__ float red[4][LA_VK];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 31, h = lane >> 5;
    const int chunk = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
    const int t0 = chunk * LA_CHUNK + wave * 64;

    // ---- stage: 8 lanes per token row (128 B), 8 rows per pass ----
    {
        const int piece = lane & 7;
        const uint16_t *src = p.kv + (long long)b * p.kv_bs + (size_t)head * 64 + piece * 8;
#pragma unroll
        for (int ps = 0; ps < 8; ps++) {
            const int tl = 8 * ps + (lane >> 3);
            v4i val = {0, 0, 0, 0};
            if (t0 + tl < p.T) val = *reinterpret_cast<const v4i *>(src + (size_t)(t0 + tl) * p.ldkv);
            if (piece < 4) val = v4i{la_relu2(val[0]), la_relu2(val[1]), la_relu2(val[2]), la_relu2(val[3])};
            *reinterpret_cast<v4i *>(&tile[wave][tl][piece * 8]) = val;
        }
    }
    __syncthreads();

    // ---- vk += V^T relu(K), 16 tokens per step ----
    v16f acc, ksum;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = ksum[r] = 0.f;
    u16x8 one8;
#pragma unroll
    for (int e = 0; e < 8; e++) one8[e] = DT == SVDQ_BF16 ? 0x3f80 : 0x3c00;
    const V8 ones = __builtin_bit_cast(V8, one8);
#pragma unroll
    for (int s = 0; s < 4; s++) {
        u16x8 vt, kt;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            kt[e] = tile[wave][16 * s + 8 * h + e][lr];
            vt[e] = tile[wave][16 * s + 8 * h + e][32 + lr];
        }
        acc = Half<DT>::mfma32(__builtin_bit_cast(V8, vt), __builtin_bit_cast(V8, kt), acc);
        ksum = Half<DT>::mfma32(ones, __builtin_bit_cast(V8, kt), ksum);
    }
#pragma unroll
    for (int r = 0; r < 16; r++) red[wave][(8 * (r >> 2) + 4 * h + (r & 3)) * 32 + lr] = acc[r];
    if (h == 0) red[wave][32 * 32 + lr] = ksum[0]; // (every row of the ones product is the column sum)
    __syncthreads();

    // ---- the chunk's partial: the waves' tiles in wave order ----
    float *dst = p.partials + (((size_t)b * p.H + head) * p.nchunks + chunk) * LA_VK;
    for (int e = tid; e < LA_VK; e += 256) dst[e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

__global__ __launch_bounds__(256) void la_finish_kernel(const float *partials, float *sums, float *vk, int nchunks, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long bh = idx / LA_VK;
    const float *src = partials + (size_t)bh * nchunks * LA_VK + (idx - bh * LA_VK);
    float s = src[0];
    for (int c = 1; c < nchunks; c++) s += src[(size_t)c * LA_VK];
    sums[idx] = s;
    if (vk) vk[idx] = s;
}

template <int DT>
__global__ __launch_bounds__(256) void la_apply_kernel(const LaParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t rows[LA_TILE * LA_QROW];
    __shared__ __attribute__((aligned(16))) float vkt[2][32 * LA_VKROW];
    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * LA_TILE, head0 = blockIdx.y * 2, b = blockIdx.z;
    const int nh = p.H - head0 < 2 ? p.H - head0 : 2;

    // ---- vk of the pair of heads, transposed: element (i, j) at [j][i] ----
    for (int u = tid; u < 2 * LA_VK; u += 256) {
        const int hh = u >= LA_VK, e = u - hh * LA_VK;
        float v = 0.f;
        if (hh < nh) v = p.sums[((size_t)b * p.H + head0 + hh) * LA_VK + e];
        vkt[hh][(e & 31) * LA_VKROW + (e >> 5)] = v;
    }
    if (tid < 192) vkt[tid / 96][(tid % 96 / 3) * LA_VKROW + 33 + tid % 3] = 0.f; // the padding the packed FMAs read
    // ---- Q rows of the pair: 8 lanes per token (128 B), 32 tokens per pass ----
    const int piece = tid & 7;
    const bool col_live = (piece >> 2) < nh;
#pragma unroll
    for (int ps = 0; ps < 4; ps++) {
        const int tl = 32 * ps + (tid >> 3);
        v4i val = {0, 0, 0, 0};
        if (col_live && t0 + tl < p.T)
            val = *reinterpret_cast<const v4i *>(p.q + (long long)b * p.q_bs + (size_t)(t0 + tl) * p.ldq + (size_t)head0 * 32 + piece * 8);
        *reinterpret_cast<v4i *>(rows + tl * LA_QROW + piece * 16) = val;
    }
    __syncthreads();

    // ---- one thread per (token, head of the pair); the head is uniform in a wave, so the vk reads are broadcasts ----
    {
        const int tl = tid & 127, hh = tid >> 7;
        uint8_t *mine = rows + tl * LA_QROW + hh * 64;
        float qf[32];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const v4i w = *reinterpret_cast<const v4i *>(mine + 16 * k);
#pragma unroll
            for (int d = 0; d < 4; d++) {
                qf[8 * k + 2 * d] = fmaxf(pk_lo<DT>((unsigned)w[d]), 0.f);
                qf[8 * k + 2 * d + 1] = fmaxf(pk_hi<DT>((unsigned)w[d]), 0.f);
            }
        }
        f32x2_t acc[17]; // (i = 2 n, 2 n + 1); acc[16] = (the denominator's sum, padding)
#pragma unroll
        for (int n = 0; n < 17; n++) acc[n] = f32x2_t{0.f, 0.f};
        const float *vh = vkt[hh];
#pragma unroll
        for (int j = 0; j < 32; j++) {
            const f32x2_t qq = {qf[j], qf[j]};
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const v4f v = *reinterpret_cast<const v4f *>(vh + j * LA_VKROW + 4 * c);
                acc[2 * c] = __builtin_elementwise_fma(f32x2_t{v[0], v[1]}, qq, acc[2 * c]);
                acc[2 * c + 1] = __builtin_elementwise_fma(f32x2_t{v[2], v[3]}, qq, acc[2 * c + 1]);
            }
            acc[16] = __builtin_elementwise_fma(*reinterpret_cast<const f32x2_t *>(vh + j * LA_VKROW + 32), qq, acc[16]);
        }
        const float inv = 1.0f / (acc[16][0] + p.eps);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v4i w;
#pragma unroll
            for (int d = 0; d < 4; d++) w[d] = (int)pack2<DT>(acc[4 * k + d][0] * inv, acc[4 * k + d][1] * inv);
            *reinterpret_cast<v4i *>(mine + 16 * k) = w; // over the thread's own Q row
        }
    }
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < 4; ps++) {
        const int tl = 32 * ps + (tid >> 3);
        if (col_live && t0 + tl < p.T)
            *reinterpret_cast<v4i *>(p.out + (long long)b * p.out_bs + (size_t)(t0 + tl) * p.ldo + (size_t)head0 * 32 + piece * 8) =
                *reinterpret_cast<const v4i *>(rows + tl * LA_QROW + piece * 16);
    }
}

static long long la_workspace_bytes(long long B, long long H, long long T) {
    return B * H * ((T + LA_CHUNK - 1) / LA_CHUNK + 1) * LA_VK * (long long)sizeof(float);
}

} // namespace svdq

using namespace svdq;

extern "C" int64_t svdq_linear_attention_workspace_bytes(const svdq_linear_attention_args *a) {
    if (!a || a->B < 1 || a->H < 1 || a->T < 1) return 0;
    return la_workspace_bytes(a->B, a->H, a->T);
}

extern "C" int svdq_linear_attention(const svdq_linear_attention_args *a, void *stream) {
    if (!a) { set_error("svdq_linear_attention: args is NULL"); return SVDQ_E_INVALID; }
    const bool apply = a->q || a->out;
    if (!a->kv || !a->workspace) { set_error("svdq_linear_attention: kv and workspace are required"); return SVDQ_E_INVALID; }
    if (apply && (!a->q || !a->out)) { set_error("svdq_linear_attention: q and out go together (both NULL: only vk)"); return SVDQ_E_INVALID; }
    if (!apply && !a->vk) { set_error("svdq_linear_attention: without q and out, vk is required"); return SVDQ_E_INVALID; }
    if (a->dtype != SVDQ_BF16 && a->dtype != SVDQ_FP16) { set_error("svdq_linear_attention: unknown dtype %d", a->dtype); return SVDQ_E_INVALID; }
    if (a->head_dim != 32) { set_error("svdq_linear_attention: head_dim=%d: only 32 is implemented", a->head_dim); return SVDQ_E_UNSUPPORTED; }
    if (a->T < 1 || a->H < 1 || a->B < 1) { set_error("svdq_linear_attention: need T=%d, H=%d, B=%d >= 1", a->T, a->H, a->B); return SVDQ_E_INVALID; }
    if (a->H > 65535 || a->B > 65535 || (long long)a->H * a->B > (1 << 20) || a->T > (1 << 30)) {
        set_error("svdq_linear_attention: H=%d, B=%d (at most 65535 each, 2^20 together) or T=%d (at most 2^30) exceeds the grid", a->H, a->B, a->T);
        return SVDQ_E_INVALID;
    }
    const long long qw = (long long)a->H * 32, kvw = (long long)a->H * 64;
    if (a->ldkv < kvw || (apply && (a->ldq < qw || a->ldo < qw))) {
        set_error("svdq_linear_attention: row strides (ldq=%d ldkv=%d ldo=%d) must be at least H * 32 = %lld for q and out, H * 64 = %lld for kv",
                  a->ldq, a->ldkv, a->ldo, qw, kvw);
        return SVDQ_E_INVALID;
    }
    if (a->B > 1) { // a batch element's rows end before the next one's begin
        const long long span = (long long)(a->T - 1);
        if (a->kv_bs < span * a->ldkv + kvw || (apply && (a->q_bs < span * a->ldq + qw || a->out_bs < span * a->ldo + qw))) {
            set_error("svdq_linear_attention: batch strides (q_bs=%lld kv_bs=%lld out_bs=%lld) must be at least (T - 1) * row stride + row width",
                      (long long)a->q_bs, (long long)a->kv_bs, (long long)a->out_bs);
            return SVDQ_E_INVALID;
        }
    }
    const uintptr_t ptrs = (uintptr_t)a->kv | (uintptr_t)a->workspace | (uintptr_t)a->vk | (uintptr_t)a->q | (uintptr_t)a->out;
    long long strides = a->ldkv | (a->B > 1 ? a->kv_bs : 0);
    if (apply) strides |= a->ldq | a->ldo | (a->B > 1 ? a->q_bs | a->out_bs : 0);
    if (ptrs & 15 || strides % 8) {
        set_error("svdq_linear_attention: q, kv, out, vk and workspace must be 16-byte aligned (pointers, and row / batch strides a multiple of 8)");
        return SVDQ_E_INVALID;
    }
    if (!(a->eps >= 0.f) || !(a->eps < INFINITY)) { set_error("svdq_linear_attention: eps must be non-negative and finite"); return SVDQ_E_INVALID; }
    const long long need = la_workspace_bytes(a->B, a->H, a->T);
    if (a->workspace_bytes < need) {
        set_error("svdq_linear_attention: workspace of %lld bytes, %lld needed (svdq_linear_attention_workspace_bytes)", (long long)a->workspace_bytes, need);
        return SVDQ_E_INVALID;
    }
    LaParams p;
    p.q = (const uint16_t *)a->q; p.kv = (const uint16_t *)a->kv; p.out = (uint16_t *)a->out; p.vk = a->vk;
    p.nchunks = (a->T + LA_CHUNK - 1) / LA_CHUNK;
    p.partials = (float *)a->workspace;
    p.sums = p.partials + (size_t)a->B * a->H * p.nchunks * LA_VK;
    p.q_bs = a->q_bs; p.kv_bs = a->kv_bs; p.out_bs = a->out_bs;
    p.ldq = a->ldq; p.ldkv = a->ldkv; p.ldo = a->ldo;
    p.T = a->T; p.H = a->H; p.eps = a->eps;
    hipStream_t st = (hipStream_t)stream;
    const bool bf = a->dtype == SVDQ_BF16;
    const dim3 rgrid(p.nchunks, a->H, a->B);
    if (bf) hipLaunchKernelGGL((la_reduce_kernel<SVDQ_BF16>), rgrid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((la_reduce_kernel<SVDQ_FP16>), rgrid, dim3(256), 0, st, p);
    const long long total = (long long)a->B * a->H * LA_VK;
    hipLaunchKernelGGL(la_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float *)p.partials, p.sums, p.vk, p.nchunks, total);
    if (apply) {
        const dim3 agrid((a->T + LA_TILE - 1) / LA_TILE, (a->H + 1) / 2, a->B);
        if (bf) hipLaunchKernelGGL((la_apply_kernel<SVDQ_BF16>), agrid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((la_apply_kernel<SVDQ_FP16>), agrid, dim3(256), 0, st, p);
    }
    return hip_check(hipGetLastError(), "svdq_linear_attention launch");
}
