// Host side of the low-rank factor's fragment image (svdq_pack_lora_down): sizes, argument validation and the index arithmetic of the layout, in plain C++
// with no HIP in it -- included by lowrank_split.h, and by tools/lowrank_image_host_check.cpp, which runs it under the host sanitizers.
//   image: [N / 16 units][nb = ceil(R2 / 32) rank blocks][64 lanes][8] 16-bit; lane (rank & 31, h), slot j <- column 16 unit + 8 (j >> 2) + 4 h + (j & 3) of
//   rank 32 block + (lane & 31); ranks >= R2: zeros.
#pragma once
#include <cstddef>
#include <cstdint>

namespace svdq {

// bytes the packed down projection(s) of a launch take ([N / 16 units][nb blocks][64 lanes][8] 16-bit per weight set)
static inline long long lowrank_split_pack_bytes(int N, int R2, bool two_sets) { return (two_sets ? 2LL : 1LL) * (N / 16) * ((R2 + 31) / 32) * 1024; }
// the split contraction behind a kernel (rank 48 .. 160)
static inline bool lowrank_split_shape_ok(int N, int R2) { return R2 > 32 && (R2 + 31) / 32 <= 5 && N % 256 == 0; }
// the attention epilogue's own low-rank pass (rank 16 / 32: one rank block, padded with zeros; N = H * 128, whole heads)
static inline bool lowrank_image_shape_ok(int N, int R2) { return R2 > 0 && R2 <= 32 && N > 0 && N % 128 == 0; }
// svdq_pack_lora_down's argument check (dtype: 0 / 1 = SVDQ_BF16 / SVDQ_FP16)
static inline bool pack_lora_down_args_ok(const void *ld, const void *out, int N, int R2, int dtype) {
    if (!ld || !out || N <= 0 || R2 <= 0 || R2 % 16 || (dtype != 0 && dtype != 1)) return false;
    return lowrank_split_shape_ok(N, R2) || lowrank_image_shape_ok(N, R2);
}
// where element (rank r, column n) of the rank-major [R2][N] factor sits in the image, in 16-bit elements
static inline long long lowrank_image_index(int R2, int n, int r) {
    const int nb = (R2 + 31) / 32, unit = n / 16, c = n % 16;
    const int h = (c >> 2) & 1, j = 4 * (c >> 3) + (c & 3), lane = 32 * h + (r & 31);
    return (((long long)unit * nb + r / 32) * 64 + lane) * 8 + j;
}
// the pack kernel and its inverse on the host (reference of the tests; `img` holds lowrank_split_pack_bytes(N, R2, false) bytes)
static inline void lowrank_image_pack_host(const uint16_t *ld, uint16_t *img, int N, int R2) {
    const long long total = lowrank_split_pack_bytes(N, R2, false) / 2;
    for (long long i = 0; i < total; i++) img[i] = 0;
    for (int r = 0; r < R2; r++)
        for (int n = 0; n < N; n++) img[lowrank_image_index(R2, n, r)] = ld[(size_t)r * N + n];
}
static inline void lowrank_image_unpack_host(const uint16_t *img, uint16_t *ld, int N, int R2) {
    for (int r = 0; r < R2; r++)
        for (int n = 0; n < N; n++) ld[(size_t)r * N + n] = img[lowrank_image_index(R2, n, r)];
}

} // namespace svdq
