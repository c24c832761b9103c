// svdq_qwen_rotary: the rotary tables of a Qwen-Image step in one launch (diffusers QwenEmbedRope.forward / _compute_video_freqs followed
// by models/qwenimage.py pack_qwen_rotary: some thirty torch ops per latent grid -- arange, polar, expand, cat, stack, pad and the
// seven-axis permute of pack_rotemb, three times over).  Every entry of every table is a copy of one (cos, sin) pair of two small per-axis
// tables that depend on theta and axes_dim alone:
//
//   pos_cs[k, c] = (cos, sin)(float(k) * inv[c]),   neg_cs[k, c] = (cos, sin)(float(-(k + 1)) * inv[c]),   k = 0 .. 4095, c = 0 .. 63
//   channels: [0, c_frame) the frame axis, [c_frame, c_frame + c_height) the height axis, the rest the width axis
//   image row r of grid g (grids back to back, a grid flattened frame-major, then height, then width), local (f, h, w):
//       frame position g + f;  height position h - (H - H / 2) with scale_rope, else h;  width likewise
//   text row t: position txt_start + t on all three axes
//
// Pure data movement: no arithmetic on a table value, so the result is bit-equal to the torch sequence run on the same axis tables.
// The STORE side is contiguous: one work item is one 16-byte piece of an output, consecutive lanes write consecutive pieces (1 KiB per wave
// instruction).  The gather side reads 8-byte pairs of tables that stay in L2 (2 MiB each).  In the packed order (models/embeddings.py
// pack_rotemb: [row tile of 16][d8][row8][pair][row half][sin, cos]) a piece holds (sin, cos) of rows r and r + 8 at one channel; in the plain
// tables (cos, sin) of two neighbouring channels of one row.  Rows between a stream's end and its 256-row boundary are zeros -- in "all" that
// includes the gap between the padded text and the image -- so a launch leaves no byte of an output unwritten.  The grid of a row comes
// from a prefix sum of at most 8 entries in the kernel arguments.  No LDS, no atomics.
#include "row_pass.h"

namespace svdq {

constexpr int QR_MAX_GRIDS = SVDQ_QWEN_ROTARY_MAX_GRIDS, QR_POS = SVDQ_QWEN_ROTARY_POSITIONS, QR_CH = 64;

struct QwenRotaryParams {
    const float2 *pos_cs, *neg_cs;
    v4f *img, *txt, *all, *img_cs, *txt_cs;
    int start[QR_MAX_GRIDS + 1]; // first image row of grid g; start[count] = image rows
    int h[QR_MAX_GRIDS], w[QR_MAX_GRIDS];
    int h_off[QR_MAX_GRIDS], w_off[QR_MAX_GRIDS]; // H - H / 2 with scale_rope, else 0
    int count, t_img, t_txt, img_pad, txt_pad, txt_start, c_frame, c_height;
    unsigned end[5]; // ends of the five outputs' piece ranges in the launch's index space (an absent output: an empty range)
};

__device__ __forceinline__ float2 qr_lookup(const QwenRotaryParams &p, int pos, int c) {
    return pos >= 0 ? p.pos_cs[(size_t)pos * QR_CH + c] : p.neg_cs[(size_t)(-pos - 1) * QR_CH + c];
}

// (cos, sin) of image row r at channel c; zeros for a padding row
__device__ __forceinline__ float2 qr_img(const QwenRotaryParams &p, int r, int c) {
    if (r >= p.t_img) return make_float2(0.f, 0.f);
    int g = 0, s = 0, H = p.h[0], W = p.w[0], ho = p.h_off[0], wo = p.w_off[0];
#pragma unroll
    for (int k = 1; k < QR_MAX_GRIDS; k++)
        if (k < p.count && r >= p.start[k]) { g = k; s = p.start[k]; H = p.h[k]; W = p.w[k]; ho = p.h_off[k]; wo = p.w_off[k]; }
    const unsigned local = (unsigned)(r - s), hw = (unsigned)H * (unsigned)W;
    const unsigned f = local / hw, rem = local - f * hw, hh = rem / (unsigned)W, ww = rem - hh * (unsigned)W;
    const int pos = c < p.c_frame ? g + (int)f : c < p.c_frame + p.c_height ? (int)hh - ho : (int)ww - wo;
    return qr_lookup(p, pos, c);
}

__device__ __forceinline__ float2 qr_txt(const QwenRotaryParams &p, int r, int c) {
    if (r >= p.t_txt) return make_float2(0.f, 0.f);
    return qr_lookup(p, p.txt_start + r, c);
}

// row r of the joint sequence [text padded to 256 | image padded to 256]
__device__ __forceinline__ float2 qr_all(const QwenRotaryParams &p, int r, int c) { return r < p.txt_pad ? qr_txt(p, r, c) : qr_img(p, r - p.txt_pad, c); }

// piece v of a packed table: [row tile of 16][d8 of 16][row8 of 8][pair of 4] -> (sin, cos) of row r, (sin, cos) of row r + 8
template <typename F> __device__ __forceinline__ v4f qr_packed_piece(unsigned v, F row_cs) {
    const int r = (int)(v >> 9) * 16 + (int)((v >> 2) & 7), c = (int)((v >> 5) & 15) * 4 + (int)(v & 3);
    const float2 lo = row_cs(r, c), hi = row_cs(r + 8, c);
    return v4f{lo.y, lo.x, hi.y, hi.x};
}
// piece v of a plain table [T, 64, (cos, sin)]: channels 2q and 2q + 1 of one row
template <typename F> __device__ __forceinline__ v4f qr_plain_piece(unsigned v, F row_cs) {
    const int r = (int)(v >> 5), c = (int)(v & 31) * 2;
    const float2 a = row_cs(r, c), b = row_cs(r, c + 1);
    return v4f{a.x, a.y, b.x, b.y};
}

__global__ __launch_bounds__(256) void qwen_rotary_kernel(const QwenRotaryParams p) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.end[4]) return;
    if (i < p.end[0]) {
        p.img[i] = qr_packed_piece(i, [&](int r, int c) { return qr_img(p, r, c); });
    } else if (i < p.end[1]) {
        const unsigned v = i - p.end[0];
        p.txt[v] = qr_packed_piece(v, [&](int r, int c) { return qr_txt(p, r, c); });
    } else if (i < p.end[2]) {
        const unsigned v = i - p.end[1];
        p.all[v] = qr_packed_piece(v, [&](int r, int c) { return qr_all(p, r, c); });
    } else if (i < p.end[3]) {
        const unsigned v = i - p.end[2];
        p.img_cs[v] = qr_plain_piece(v, [&](int r, int c) { return qr_img(p, r, c); });
    } else {
        const unsigned v = i - p.end[3];
        p.txt_cs[v] = qr_plain_piece(v, [&](int r, int c) { return qr_txt(p, r, c); });
    }
}

} // namespace svdq

using namespace svdq;

extern "C" int svdq_qwen_rotary(const svdq_qwen_rotary_args *a, void *stream) {
    const char *op = "svdq_qwen_rotary";
    if (!a) { set_error("%s: args is NULL", op); return SVDQ_E_INVALID; }
    if (!a->pos_cs || !a->neg_cs) { set_error("%s: the axis tables pos_cs and neg_cs are required", op); return SVDQ_E_INVALID; }
    if (a->count < 1 || a->count > QR_MAX_GRIDS) { set_error("%s: count=%d grids: 1 .. %d are supported", op, a->count, QR_MAX_GRIDS); return SVDQ_E_INVALID; }
    if (a->c_frame < 0 || a->c_height < 0 || a->c_frame + a->c_height > QR_CH) {
        set_error("%s: c_frame=%d and c_height=%d must be >= 0 and leave the width axis the rest of %d channels", op, a->c_frame, a->c_height, QR_CH);
        return SVDQ_E_INVALID;
    }
    if (a->txt_len < 0 || a->txt_start < 0 || (long long)a->txt_start + a->txt_len > QR_POS) {
        set_error("%s: txt_len=%d and txt_start=%d must be >= 0 and the last text position txt_start + txt_len - 1 below %d", op, a->txt_len, a->txt_start, QR_POS);
        return SVDQ_E_INVALID;
    }
    if (!aligned_to(16, {a->pos_cs, a->neg_cs, a->img, a->txt, a->all, a->img_cs, a->txt_cs})) {
        set_error("%s: the axis tables and the outputs must be 16-byte aligned", op);
        return SVDQ_E_INVALID;
    }
    QwenRotaryParams p = {};
    const bool scale = a->scale_rope != 0;
    long long rows = 0;
    for (int g = 0; g < a->count; g++) {
        const long long F = a->grids[3 * g], H = a->grids[3 * g + 1], W = a->grids[3 * g + 2];
        if (F < 1 || H < 1 || W < 1) { set_error("%s: grid %d = (%lld, %lld, %lld): every extent must be >= 1", op, g, F, H, W); return SVDQ_E_INVALID; }
        // the positions the launch reads: frame g .. g + F - 1; height / width -(n - n / 2) .. n / 2 - 1 with scale_rope (row k of neg_cs is -(k + 1)), else 0 .. n - 1
        const long long reach = scale ? (H > W ? H : W) - (H > W ? H : W) / 2 : (H > W ? H : W);
        if (g + F > QR_POS || reach > QR_POS) {
            set_error("%s: grid %d = (%lld, %lld, %lld) reads a position at or beyond %d (the axis tables hold %d positions per sign)", op, g, F, H, W, QR_POS, QR_POS);
            return SVDQ_E_INVALID;
        }
        p.start[g] = (int)rows;
        p.h[g] = (int)H; p.w[g] = (int)W;
        p.h_off[g] = scale ? (int)(H - H / 2) : 0; p.w_off[g] = scale ? (int)(W - W / 2) : 0;
        rows += F * H * W; // (at most 2^36 per grid: no overflow)
        if (rows > SVDQ_QWEN_ROTARY_MAX_ROWS) break;
    }
    const long long txt_pad = ((long long)a->txt_len + 255) / 256 * 256, img_pad = (rows + 255) / 256 * 256;
    // one work item per 16-byte piece, indexed in 32 bits: at most 96 pieces per padded row over the five outputs
    if (rows > SVDQ_QWEN_ROTARY_MAX_ROWS || img_pad + txt_pad > SVDQ_QWEN_ROTARY_MAX_ROWS) {
        set_error("%s: %lld image rows + %d text rows: at most %d rows (padded to 256 per stream) are addressed in 32 bits", op, rows, a->txt_len, SVDQ_QWEN_ROTARY_MAX_ROWS);
        return SVDQ_E_INVALID;
    }
    // (the pointers' alignment was checked above, before the grids)
    if (!a->img && !a->txt && !a->all && !a->img_cs && !a->txt_cs) { set_error("%s: one of img / txt / all / img_cs / txt_cs is required", op); return SVDQ_E_INVALID; }
    p.start[a->count] = (int)rows;
    p.pos_cs = (const float2 *)a->pos_cs; p.neg_cs = (const float2 *)a->neg_cs;
    p.img = (v4f *)a->img; p.txt = (v4f *)a->txt; p.all = (v4f *)a->all; p.img_cs = (v4f *)a->img_cs; p.txt_cs = (v4f *)a->txt_cs;
    p.count = a->count; p.t_img = (int)rows; p.t_txt = a->txt_len; p.img_pad = (int)img_pad; p.txt_pad = (int)txt_pad;
    p.txt_start = a->txt_start; p.c_frame = a->c_frame; p.c_height = a->c_height;
    const long long pieces[5] = {a->img ? img_pad * 32 : 0, a->txt ? txt_pad * 32 : 0, a->all ? (txt_pad + img_pad) * 32 : 0, a->img_cs ? rows * 32 : 0,
                                 a->txt_cs ? (long long)a->txt_len * 32 : 0};
    long long end = 0;
    for (int k = 0; k < 5; k++) { end += pieces[k]; p.end[k] = (unsigned)end; }
    if (end == 0) return SVDQ_OK; // (only empty outputs were asked for: txt / txt_cs at txt_len = 0)
    hipLaunchKernelGGL(qwen_rotary_kernel, dim3((unsigned)((end + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return hip_check(hipGetLastError(), "svdq_qwen_rotary launch");
}
