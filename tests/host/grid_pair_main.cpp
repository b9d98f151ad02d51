// Stand-alone driver of the HOST pairings built on csrc/persist_common.h (mvd_h0_pair_host of csrc/persist.hip and
// mvd_cub3d_pair_host of csrc/cubical3d.hip), for sanitizer runs of that code outside Python.  It builds the grid-edge keys
// of a small field with heavy ties by the documented formula, sorts them, pairs conn 6 and 26 at both signs and cubical
// dimensions 0 and 2 (two samples on two threads), checks the invariants of the results and that the two refused inputs --
// keys that do not ascend, a slot index past V * n_off -- come back as errors.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       tests/host/grid_pair_main.cpp multimodal_mvd_seg_amd/csrc/persist.hip multimodal_mvd_seg_amd/csrc/cubical3d.hip \
//       multimodal_mvd_seg_amd/csrc/topo.hip multimodal_mvd_seg_amd/csrc/common.hip -o grid_pair_main && ./grid_pair_main
//
// No device call is made.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mvdseg_hip.h"

static const int D = 5, H = 6, W = 7;
static const long V = (long)D * H * W;

static uint32_t ord(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// half-neighbourhoods in the library's enumeration; outside: one more slot, the edge of a border voxel to the outside
static std::vector<std::vector<int>> offsets(int conn) {
    std::vector<std::vector<int>> o;
    if (conn == 6) return {{0, 0, 1}, {0, 1, 0}, {1, 0, 0}};
    for (int dz = 0; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++)
                if (!(dz == 0 && (dy < 0 || (dy == 0 && dx <= 0)))) o.push_back({dz, dy, dx});
    return o;
}

static std::vector<uint64_t> sorted_keys(const float *f, int conn, bool negate, bool outside) {
    const auto off = offsets(conn);
    const long n = (long)off.size() + (outside ? 1 : 0);
    auto g = [&](long v) {
        const float x = negate ? -f[v] : f[v];
        return x == 0.f ? 0.f : x;
    };
    std::vector<uint64_t> keys;
    for (int z = 0; z < D; z++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const long v = ((long)z * H + y) * W + x;
                for (long k = 0; k < (long)off.size(); k++) {
                    const int zz = z + off[k][0], yy = y + off[k][1], xx = x + off[k][2];
                    if (zz < 0 || zz >= D || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                    const long u = ((long)zz * H + yy) * W + xx;
                    keys.push_back(((uint64_t)ord(std::max(g(v), g(u))) << 32) | (uint64_t)(v * n + k));
                }
                if (outside && (x == 0 || x == W - 1 || y == 0 || y == H - 1 || z == 0 || z == D - 1))
                    keys.push_back(((uint64_t)ord(g(v)) << 32) | (uint64_t)(v * n + n - 1));
            }
    std::sort(keys.begin(), keys.end());
    return keys;
}

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main() {
    std::vector<float> f((size_t)(2 * V));
    uint32_t s = 12345u;
    for (long i = 0; i < 2 * V; i++) {
        s = s * 1664525u + 1013904223u;
        f[i] = roundf(((float)(s >> 8) / (float)(1 << 24) * 4.f - 2.f) * 2.f) / 2.f;  // halves: heavy ties, zeros
    }
    f[3] = -0.0f;
    std::vector<float> death((size_t)V);
    std::vector<int64_t> dv((size_t)V);
    for (int conn : {6, 26})
        for (int sublevel = 1; sublevel >= 0; sublevel--) {
            const auto keys = sorted_keys(f.data(), conn, !sublevel, false);
            CHECK((long)keys.size() == mvd_h0_num_edges(D, H, W, conn));
            CHECK(mvd_h0_pair_host(f.data(), keys.data(), (long)keys.size(), D, H, W, conn, sublevel, death.data(), dv.data()) == 1);
            long essential = 0;
            for (long v = 0; v < V; v++) {
                if (dv[v] < 0) {
                    essential += std::isinf(death[v]) ? 1 : 100;
                    continue;
                }
                CHECK(dv[v] < V && f[dv[v]] == death[v]);                            // the death is the critical vertex's value
                CHECK(sublevel ? death[v] >= f[v] : death[v] <= f[v]);
            }
            CHECK(essential == 1);
            printf("h0 conn %d %s: ok\n", conn, sublevel ? "sub" : "super");
        }
    std::vector<int32_t> bars((size_t)(2 * V * 2)), counts(2);
    for (int dim : {0, 2}) {
        std::vector<uint64_t> keys;
        long nv = -1, per = 0;
        CHECK(mvd_cub3d_num_keys(D, H, W, dim, &nv) == V * (dim == 2 ? 4 : 13));
        for (int n = 0; n < 2; n++) {
            const auto k = sorted_keys(f.data() + n * V, dim == 2 ? 6 : 26, dim == 2, dim == 2);
            per = (long)k.size();
            keys.insert(keys.end(), k.begin(), k.end());
        }
        CHECK(per == nv);
        CHECK(mvd_cub3d_pair_host(f.data(), keys.data(), per, 2, D, H, W, dim, bars.data(), counts.data(), 2) == 0);
        for (int n = 0; n < 2; n++) {
            CHECK(counts[n] >= 0 && counts[n] <= V);
            for (long r = 0; r < counts[n]; r++) {
                const int32_t b = bars[(n * V + r) * 2], d = bars[(n * V + r) * 2 + 1];
                CHECK(b >= 0 && b < V && d >= 0 && d < V && f[n * V + b] < f[n * V + d]);
            }
        }
        printf("cubical dimension %d: %d + %d bars\n", dim, counts[0], counts[1]);
    }
    // the refusals: the right number of keys, but no sorted filtration of the grid
    const auto good = sorted_keys(f.data(), 6, false, false);
    auto swapped = good, past = good;
    std::swap(swapped.front(), swapped.back());
    past.back() = (past.back() & 0xffffffff00000000ull) | (uint64_t)(V * 3);
    CHECK(mvd_h0_pair_host(f.data(), swapped.data(), (long)good.size(), D, H, W, 6, 1, death.data(), dv.data()) < 0);
    CHECK(strlen(mvd_last_error()) > 0);
    CHECK(mvd_h0_pair_host(f.data(), past.data(), (long)good.size(), D, H, W, 6, 1, death.data(), dv.data()) < 0);
    CHECK(mvd_h0_pair_host(f.data(), good.data(), (long)good.size(), D, H, W, 6, 1, death.data(), dv.data()) == 1);
    printf("ok\n");
    return 0;
}
