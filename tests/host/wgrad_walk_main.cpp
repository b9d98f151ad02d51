// The tile walk of k_wgrad_wino3 (conv_geom.h: tile_walk_at, tile_walk_advance) against plain division.
//   * small extents, 1 included: every split count 1..ntiles, every split, every tile a split visits and the one past
//     the last (the kernel builds that one's empty descriptors);
//   * a grid at the entry point's limit of 2^30 tiles, walked from a few splits with large strides.
// Prints "ok <tiles compared>" or the first mismatch; tests/test_wgrad_wino3_walk_host.py runs it.
#include "conv_geom.h"

#include <stdio.h>

using namespace mvd;

static long long compared = 0;

static bool same(const TileWalk &p, long long tile, int ntw, int nth, int ntd) {
    compared++;
    const long long tw = tile % ntw, th = tile / ntw % nth, td = tile / ntw / nth % ntd, n = tile / ntw / nth / ntd;
    if (p.tw == tw && p.th == th && p.td == td && p.n == n) return true;
    printf("mismatch at tile %lld of %d x %d x %d: walk (%d, %d, %d, %d), division (%lld, %lld, %lld, %lld)\n", tile, ntw, nth,
           ntd, p.tw, p.th, p.td, p.n, tw, th, td, n);
    return false;
}

// the kernel's loop: the split's first tile by division, then one advance per tile, the tile past the end included
static bool walk(int N, int ntw, int nth, int ntd, long long nsplit, long long split) {
    const long long ntiles = (long long)N * ntd * nth * ntw;
    const TileWalk step = tile_walk_at((int)nsplit, ntw, nth, ntd);
    if (step.tw >= ntw || step.th >= nth || step.td >= ntd) {
        printf("step digit out of range for nsplit %lld\n", nsplit);
        return false;
    }
    TileWalk pos = tile_walk_at((int)split, ntw, nth, ntd);
    long long tile = split;
    if (!same(pos, tile, ntw, nth, ntd)) return false;
    while (tile < ntiles) {
        tile += nsplit;
        tile_walk_advance(pos, step, ntw, nth, ntd);
        if (!same(pos, tile, ntw, nth, ntd)) return false;
    }
    return true;
}

int main() {
    const int EXT[][4] = {{1, 1, 1, 1}, {3, 1, 1, 1}, {1, 1, 1, 5}, {2, 2, 2, 3}, {3, 1, 2, 2}, {1, 5, 1, 3}, {2, 3, 4, 1}, {2, 7, 3, 2}};
    for (const auto &e : EXT) {  // N, ntw, nth, ntd
        const long long ntiles = (long long)e[0] * e[1] * e[2] * e[3];
        for (long long nsplit = 1; nsplit <= ntiles; nsplit++)
            for (long long split = 0; split < nsplit; split++)
                if (!walk(e[0], e[1], e[2], e[3], nsplit, split)) return 1;
    }
    // 2^30 tiles (the limit of wgrad_wino3): 4 x (64 x 64 x 65536), and a ragged one just below it
    const int BIG[][4] = {{4, 64, 64, 65536}, {3, 61, 127, 46199}};
    const long long NSPLIT[] = {256, 4099, 1000003};
    for (const auto &e : BIG)
        for (long long nsplit : NSPLIT)
            for (long long split : {0LL, 1LL, nsplit / 2, nsplit - 1})
                if (!walk(e[0], e[1], e[2], e[3], nsplit, split)) return 1;
    printf("ok %lld\n", compared);
    return 0;
}
