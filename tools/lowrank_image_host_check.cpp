// Host-only check of the low-rank factor's fragment image (nunchaku_amd/csrc/lowrank_image_host.h: what svdq_pack_lora_down(_bytes) and svdq_attention
// decide on the host): sizes, argument validation, and the layout's index arithmetic -- pack then unpack is the identity, every image element is written at
// most once, the padding stays zero, and fragment (unit, lane) holds the eight values the attention epilogue's two row-per-lane 8-byte loads fetch.
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/lowrank_image_host_check.cpp -o lowrank_image_host_check && ./lowrank_image_host_check
// (heap buffers of exactly the queried size: an index beyond the image is an AddressSanitizer report)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../nunchaku_amd/csrc/lowrank_image_host.h"

using namespace svdq;

static int fails = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("line %d: %s\n", __LINE__, #c);             \
            fails++;                                                \
        }                                                           \
    } while (0)

static void roundtrip(int N, int R2) {
    const long long bytes = lowrank_split_pack_bytes(N, R2, false);
    CHECK(bytes == (long long)(N / 16) * ((R2 + 31) / 32) * 1024);
    uint16_t *ld = (uint16_t *)std::malloc((size_t)R2 * N * 2), *back = (uint16_t *)std::malloc((size_t)R2 * N * 2);
    uint16_t *img = (uint16_t *)std::malloc((size_t)bytes);
    for (long long i = 0; i < (long long)R2 * N; i++) ld[i] = (uint16_t)(1 + (i * 2654435761u >> 7) % 65535); // never 0: the padding is told apart
    lowrank_image_pack_host(ld, img, N, R2);
    lowrank_image_unpack_host(img, back, N, R2);
    long long bad = 0, nonzero = 0;
    for (long long i = 0; i < (long long)R2 * N; i++) bad += back[i] != ld[i];
    for (long long i = 0; i < bytes / 2; i++) nonzero += img[i] != 0;
    CHECK(bad == 0);
    CHECK(nonzero == (long long)R2 * N); // a bijection onto the live part; ranks >= R2 zero
    // the attention epilogue's pass (rank <= 32): lane (lr, h) of step (dt, qq) of head `head` reads 4 + 4 values at rank row lr, columns
    // head * 128 + dt * 32 + qq * 16 + h * 4 (+ 8); the image holds them as the lane's 8 slots of unit head * 8 + dt * 2 + qq
    if (R2 <= 32 && N % 128 == 0) {
        long long wrong = 0;
        for (int head = 0; head < N / 128; head++)
            for (int step = 0; step < 8; step++)
                for (int lane = 0; lane < 64; lane++) {
                    const int lr = lane & 31, h = lane >> 5, dt = step >> 1, qq = step & 1;
                    const uint16_t *frag = img + ((size_t)(head * 8 + step) * 64 + lane) * 8;
                    for (int j = 0; j < 8; j++) {
                        const int col = head * 128 + dt * 32 + qq * 16 + h * 4 + (j & 3) + 8 * (j >> 2);
                        const uint16_t want = lr < R2 ? ld[(size_t)lr * N + col] : 0;
                        wrong += frag[j] != want;
                    }
                }
        CHECK(wrong == 0);
    }
    std::free(ld); std::free(back); std::free(img);
}

int main() {
    int a = 0, b = 0; // any non-null pointers: the validation does not look behind them
    const void *ld = &a;
    void *out = &b;
    // shapes: the split contraction's (48 .. 160, N % 256) and the attention epilogue's (16 / 32, N % 128)
    for (int R2 = -16; R2 <= 272; R2 += 8)
        for (int N : {-128, 0, 16, 64, 128, 256, 384, 3072, 3080}) {
            const bool want = R2 > 0 && R2 % 16 == 0 && N > 0 &&
                              ((R2 >= 48 && R2 <= 160 && N % 256 == 0) || (R2 <= 32 && N % 128 == 0));
            CHECK(pack_lora_down_args_ok(ld, out, N, R2, 0) == want);
            CHECK(pack_lora_down_args_ok(ld, out, N, R2, 1) == want);
            CHECK(!pack_lora_down_args_ok(nullptr, out, N, R2, 0));
            CHECK(!pack_lora_down_args_ok(ld, nullptr, N, R2, 0));
            CHECK(!pack_lora_down_args_ok(ld, out, N, R2, 2));
            CHECK(!pack_lora_down_args_ok(ld, out, N, R2, -1));
        }
    CHECK(lowrank_split_pack_bytes(3072, 32, false) == 196608 && lowrank_split_pack_bytes(3072, 16, false) == 196608); // one rank block, padded
    CHECK(lowrank_split_pack_bytes(3072, 128, true) == 2LL * 192 * 4 * 1024);
    CHECK(lowrank_split_pack_bytes(0x7ffffff0, 160, true) == 2LL * (0x7ffffff0 / 16) * 5 * 1024); // no 32-bit overflow
    CHECK(!lowrank_image_shape_ok(3072, 48) && lowrank_image_shape_ok(384, 16) && !lowrank_split_shape_ok(3072, 32));
    for (int R2 : {16, 32, 48, 128, 160})
        for (int N : {256, 3072}) roundtrip(N, R2);
    roundtrip(384, 16);
    roundtrip(128, 32);
    std::printf("lowrank image host check: %d failures\n", fails);
    return fails ? 1 : 0;
}
