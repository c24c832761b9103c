// Host-only replay of launch_quantize's grid rule (nunchaku_amd/csrc/quantize.hip): chunks per workgroup `cpw` and K slices for a launch of
// tiles = M_pad / 32 row tiles and KP = K / 128 chunks.  Compares the rule before the fix (doubling while tiles * ceil(KP / cpw) > 8192: never ends
// once tiles > 8192, cpw overflows) with the current one (doubling stops at cpw >= KP) over every tiles = 8 .. 8192 (step 8: M_pad is a multiple
// of 256) and KP = 1 .. 128 -- the choice must not change for any M_pad <= 262144 -- and runs the current rule beyond.
//   c++ -O1 -fsanitize=undefined -fno-sanitize-recover=undefined tools/quantize_grid_rule.cpp -o quantize_grid_rule && ./quantize_grid_rule
// (old_rule is only ever called where it terminates.)
#include <cstdio>

struct Grid { int cpw, slices; };

static Grid old_rule(int tiles, int KP) {
    int cpw = 4;
    while ((long)tiles * ((KP + cpw - 1) / cpw) > 8192) cpw *= 2;
    if (cpw > KP) cpw = ((KP + 3) / 4) * 4;
    return {cpw, (KP + cpw - 1) / cpw};
}

static Grid new_rule(int tiles, int KP) {
    int cpw = 4;
    while (cpw < KP && (long)tiles * ((KP + cpw - 1) / cpw) > 8192) cpw *= 2;
    if (cpw > KP) cpw = ((KP + 3) / 4) * 4;
    return {cpw, (KP + cpw - 1) / cpw};
}

int main() {
    long compared = 0, differ = 0;
    for (int tiles = 8; tiles <= 8192; tiles += 8)
        for (int KP = 1; KP <= 128; KP++) {
            const Grid a = old_rule(tiles, KP), b = new_rule(tiles, KP);
            compared++;
            if (a.cpw != b.cpw || a.slices != b.slices) {
                if (differ++ < 10) std::printf("tiles=%d KP=%d: old cpw=%d slices=%d, new cpw=%d slices=%d\n", tiles, KP, a.cpw, a.slices, b.cpw, b.slices);
            }
        }
    long beyond = 0, bad = 0;
    for (int tiles = 8200; tiles <= 1 << 20; tiles += 8 * 97)
        for (int KP = 1; KP <= 128; KP++) {
            const Grid b = new_rule(tiles, KP);
            beyond++;
            if (b.cpw < 4 || b.cpw % 4 || b.slices < 1 || (long)b.slices * b.cpw < KP || (long)(b.slices - 1) * b.cpw >= KP) bad++;
        }
    std::printf("%ld (tiles, KP) pairs up to 8192 row tiles: %ld differ; %ld pairs beyond: %ld without a covering grid\n", compared, differ, beyond, bad);
    return differ || bad ? 1 : 0;
}
