// Stand-alone driver of the HOST pairing of csrc/levelset2d.hip (mvd_ls2d_pair_host), for sanitizer runs of that code
// outside Python.  It builds the cell keys of a W x H field by the documented formula, sorts them, pairs two problems
// (the field and its negative) on two threads and checks the invariants of the result.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       tests/host/ls2d_pair_main.cpp multimodal_mvd_seg_amd/csrc/levelset2d.hip multimodal_mvd_seg_amd/csrc/common.hip \
//       -o ls2d_pair_main && ./ls2d_pair_main 7 9 1 && ./ls2d_pair_main 1 5 0
//
// arguments: W H quarters (1: values rounded to quarters = heavy ties).  No device call is made.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mvdseg_hip.h"

static uint32_t ord(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

int main(int argc, char **argv) {
    const int W = argc > 1 ? atoi(argv[1]) : 7, H = argc > 2 ? atoi(argv[2]) : 9, quarters = argc > 3 ? atoi(argv[3]) : 1;
    long V, E, T;
    const long n = mvd_ls2d_num_cells(H, W, 1, &V, &E, &T);
    if (n < 0) return 2;
    std::vector<float> f((size_t)V);
    uint32_t s = 12345u;
    for (long i = 0; i < V; i++) {
        s = s * 1664525u + 1013904223u;
        float v = (float)(s >> 8) / (float)(1 << 24) * 4.f - 2.f;
        f[i] = quarters ? roundf(v * 4.f) / 4.f : v;
    }
    std::vector<uint64_t> keys((size_t)(2 * n));
    for (int p = 0; p < 2; p++) {
        auto g = [&](long v) {
            float x = p ? -f[v] : f[v];
            return x == 0.f ? 0.f : x;
        };
        uint64_t *k = keys.data() + p * n;
        long c = 0;
        for (long v = 0; v < V; v++) k[c++] = ((uint64_t)ord(g(v)) << 32) | (uint64_t)v;
        long e = 0;
        auto edge = [&](long a, long b) { k[c++] = ((uint64_t)ord(std::max(g(a), g(b))) << 32) | (1u << 30) | (uint64_t)e++; };
        for (int i = 0; i < H; i++)
            for (int j = 0; j + 1 < W; j++) edge((long)i * W + j, (long)i * W + j + 1);
        for (int i = 0; i + 1 < H; i++)
            for (int j = 0; j < W; j++) edge((long)i * W + j, (long)(i + 1) * W + j);
        for (int i = 0; i + 1 < H; i++)
            for (int j = 0; j + 1 < W; j++) edge((long)i * W + j, (long)(i + 1) * W + j + 1);
        long t = 0;
        for (int i = 0; i + 1 < H; i++)
            for (int j = 0; j + 1 < W; j++) {
                const long a = (long)i * W + j, d = a + W + 1;
                for (long b : {a + 1, a + W})
                    k[c++] = ((uint64_t)ord(std::max(g(a), std::max(g(b), g(d)))) << 32) | (2u << 30) | (uint64_t)t++;
            }
        if (c != n || e != E || t != T) return 3;
        std::sort(k, k + n);
    }
    std::vector<int32_t> bars((size_t)(2 * (V + T) * 4)), er((size_t)(2 * std::max(E, 1L)));
    // problem 0 is the sub-level filtration of f; problem 1, keyed on -f, is its super-level filtration when paired as such
    for (int sublevel = 1; sublevel >= 0; sublevel--) {
        const uint64_t *k = keys.data() + (sublevel ? 0 : n);
        std::vector<uint64_t> two(k, k + n);
        two.insert(two.end(), k, k + n);
        if (mvd_ls2d_pair_host(two.data(), 2, H, W, sublevel, 1, bars.data(), er.data(), 2) != 0) {
            fprintf(stderr, "pair_host failed: %s\n", mvd_last_error());
            return 1;
        }
        long essential = 0, nonzero1 = 0;
        for (long r = 0; r < V + T; r++) {
            const int32_t *row = bars.data() + 4 * r, *row2 = row + 4 * (V + T);
            if (memcmp(row, row2, 16)) return 4;   // the two threads paired the same problem the same way
            float b, d;
            memcpy(&b, row, 4);
            memcpy(&d, row + 1, 4);
            if (row[2] < 0 || row[2] >= V || f[row[2]] != b) return 5;
            if (row[3] >= V || (row[3] >= 0 && f[row[3]] != d)) return 6;
            if (row[3] < 0) essential += (r < V && std::isinf(d)) ? 1 : 100;
            if (r >= V && b != d) nonzero1++;
        }
        if (essential != 1) return 7;
        printf("%dx%d %s: %ld + %ld bars, %ld of non-zero length in dimension 1\n", W, H, sublevel ? "sub" : "super", V, T, nonzero1);
    }
    printf("ok\n");
    return 0;
}
