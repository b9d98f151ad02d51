// What the grid-persistence pipelines share (persist.hip: H0 of a 3-D field; cubical3d.hip: cubical dimensions 0 and 2;
// levelset2d.hip: H0 + H1 on the Freudenthal plane; topo.hip: connected components): the half-neighbourhood table, the
// order-preserving key of a float, the grid-edge key kernel, the u64 radix sort out of a workspace, the elder-rule sweep
// over sorted grid-edge keys and the host thread pool.
//
// The TIE RULES live here and nowhere else in csrc/ (oracle/cc_oracle.c and tests/*_ref.py restate them independently):
//   vertices are ordered by (g value, linear index), g = f or -f with -0 folded to +0;
//   edges by (max(g[v], g[u]), v * n_off + k), k = the slot in the half-neighbourhood enumeration below;
//   the critical vertex of an edge is the arg-max of g, v on ties.
#pragma once
#include "common.h"

#include <hipcub/hipcub.hpp>

#include <new>
#include <thread>
#include <vector>

namespace mvd {

struct GridOffsets {
    int n;        // slots per voxel
    int outside;  // the slot that is the edge to the outside vertex (cubical dimension 2), or -1
    int off[13][3];
};

// half-neighbourhood (each undirected edge once), same enumeration as oracle/cc_oracle.c::neighbour_offsets
static inline int grid_half_offsets(int conn, GridOffsets *o) {
    o->n = 0;
    o->outside = -1;
    if (conn == 6) {
        const int t[3][3] = {{0, 0, 1}, {0, 1, 0}, {1, 0, 0}};
        for (int i = 0; i < 3; i++) memcpy(o->off[o->n++], t[i], sizeof(int) * 3);
    } else if (conn == 14) {
        const int t[7][3] = {{0, 0, 1}, {0, 1, 0}, {1, 0, 0}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}, {1, 1, 1}};
        for (int i = 0; i < 7; i++) memcpy(o->off[o->n++], t[i], sizeof(int) * 3);
    } else if (conn == 26) {
        for (int dz = 0; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    if (dz == 0 && (dy < 0 || (dy == 0 && dx <= 0))) continue;
                    o->off[o->n][0] = dz;
                    o->off[o->n][1] = dy;
                    o->off[o->n][2] = dx;
                    o->n++;
                }
    } else {
        return 1;
    }
    return 0;
}

// the slots that are edges: grid edges that stay in the grid, plus one outside edge per border voxel
static inline long grid_valid_edges(int D, int H, int W, const GridOffsets &o) {
    long n = 0;
    for (int k = 0; k < o.n; k++) {
        if (k == o.outside) continue;
        const long a = D - abs(o.off[k][0]), b = H - abs(o.off[k][1]), c = W - abs(o.off[k][2]);
        if (a > 0 && b > 0 && c > 0) n += a * b * c;
    }
    if (o.outside >= 0) {
        const long a = D > 2 ? D - 2 : 0, b = H > 2 ? H - 2 : 0, c = W > 2 ? W - 2 : 0;
        n += (long)D * H * W - a * b * c;
    }
    return n;
}

// monotone map float -> uint32 (a < b  <=>  key(a) < key(b)); -0.0 is canonicalised to +0.0 by fold_sign
__host__ __device__ inline uint32_t f2ord(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ord2f(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float v;
    memcpy(&v, &u, 4);
    return v;
}
// g of the header: a sweep downwards in f (super-level sets, cubical dimension 2) is the sweep upwards in -f
__host__ __device__ inline float fold_sign(float v, int negate) {
    float g = negate ? -v : v;
    return g == 0.f ? 0.f : g;
}

static inline long ew_blocks(long n, long cap) {
    long b = cdiv(n, 256);
    return b > cap ? cap : (b < 1 ? 1 : b);
}

// one thread per (voxel, slot): key = ord(max(g[v], g[u])) << 32 | (v * n_off + k); the outside edge of a border voxel
// has the value max(g[v], -inf) = g[v]; slots that leave the grid get the all-ones key and sort to the end (their number
// is known on the host: grid_valid_edges)
static __global__ void k_grid_edge_keys(const float *__restrict__ f, uint64_t *__restrict__ keys, int D, int H, int W,
                                        const GridOffsets o, int negate) {
    const long V = (long)D * H * W, total = V * o.n;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long v = e / o.n;
        const int k = (int)(e - v * o.n);
        const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((long)W * H));
        uint64_t key = ~0ull;
        if (k == o.outside) {
            if (x == 0 || x == W - 1 || y == 0 || y == H - 1 || z == 0 || z == D - 1)
                key = ((uint64_t)f2ord(fold_sign(f[v], negate)) << 32) | (uint64_t)e;
        } else {
            const int zz = z + o.off[k][0], yy = y + o.off[k][1], xx = x + o.off[k][2];
            if (zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const long u = ((long)zz * H + yy) * W + xx;
                const float a = fold_sign(f[v], negate), b = fold_sign(f[u], negate);
                key = ((uint64_t)f2ord(a < b ? b : a) << 32) | (uint64_t)e;
            }
        }
        keys[e] = key;
    }
}

// workspace layout of a u64 radix sort: [n unsorted keys][pad to 256 bytes][hipCUB's temporary storage]
static inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }
static inline size_t sort_u64_temp_bytes(long n) {
    size_t t = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, t, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)n, 0, 64);
    return t;
}
static inline size_t sort_u64_workspace_bytes(long n) { return al256((size_t)n * sizeof(uint64_t)) + sort_u64_temp_bytes(n) + 512; }
// sorts the n keys at the start of ws into `sorted`
static inline hipError_t sort_u64_from_workspace(void *ws, size_t ws_bytes, long n, uint64_t *sorted, hipStream_t s) {
    const size_t koff = al256((size_t)n * sizeof(uint64_t));
    size_t temp_bytes = ws_bytes - koff;
    return hipcub::DeviceRadixSort::SortKeys(reinterpret_cast<char *>(ws) + koff, temp_bytes,
                                             reinterpret_cast<const uint64_t *>(ws), sorted, (int)n, 0, 64, s);
}

// path-halving find of the host union-finds
static inline int32_t uf_find(int32_t *p, int32_t x) {
    while (p[x] != x) {
        p[x] = p[p[x]];
        x = p[x];
    }
    return x;
}

// Elder-rule union-find sweep over the n_keys sorted grid-edge keys of ONE field f (as given, not sign-flipped).  Every
// edge that joins two components calls emit(young, crit, val): the component founded at vertex `young` dies at this edge,
// whose critical vertex is `crit` and whose value is val = g[crit].  With an outside slot, vertex V is the outside: older
// than every voxel, and never the critical vertex of its edges.  Returns the number of merges, or -1 for keys that are no
// sorted filtration of this grid (not ascending, a slot >= V * n, a neighbour outside [0, V)) or without host memory.
// NEG is `negate` at compile time: the comparisons below then are plain comparisons of f, in either direction.
template <bool NEG, class Emit>
static inline long grid_elder_sweep_signed(const float *f, const uint64_t *keys, long n_keys, int D, int H, int W,
                                           const GridOffsets &o, Emit emit) {
    const long V = (long)D * H * W;
    const int32_t OUT = (int32_t)V;
    std::vector<int32_t> p;
    try {
        p.resize((size_t)V + 1);
    } catch (const std::bad_alloc &) {
        return -1;
    }
    for (long i = 0; i <= V; i++) p[(size_t)i] = (int32_t)i;
    long doff[13];
    for (int k = 0; k < o.n; k++) doff[k] = ((long)o.off[k][0] * H + o.off[k][1]) * W + o.off[k][2];
    const uint64_t total = (uint64_t)V * (uint64_t)o.n;
    const auto g = [&](long i) { return NEG ? -f[i] : f[i]; };  // -0 == +0: only the value handed out needs the fold
    long merges = 0, alive = o.outside >= 0 ? V + 1 : V;
    for (long e = 0; e < n_keys; e++) {
        const uint64_t key = keys[e];
        const uint32_t idx = (uint32_t)key;
        if ((e > 0 && key < keys[e - 1]) || (uint64_t)idx >= total) return -1;
        if (alive <= 1) continue;  // everything is one component: the rest of the keys is only checked
        const long v = idx / (uint32_t)o.n;
        const int k = (int)(idx - (uint32_t)v * (uint32_t)o.n);
        const bool outside = k == o.outside;
        const long u = outside ? V : v + doff[k];
        if (u < 0 || u > V || (!outside && u >= V)) return -1;
        const int32_t a = uf_find(p.data(), (int32_t)v), b = uf_find(p.data(), (int32_t)u);
        if (a == b) continue;  // the edge closes a 1-cycle: not an H0 event
        // filtration rank of a vertex = (value, index); the outside vertex is the eldest
        const bool a_younger = b == OUT || (a != OUT && (g(a) > g(b) || (g(a) == g(b) && a > b)));
        const int32_t young = a_younger ? a : b, old = a_younger ? b : a;
        const int32_t crit = (int32_t)((!outside && g(v) < g(u)) ? u : v);  // complex.cpp:141-145: the arg-max vertex
        emit(young, crit, fold_sign(f[crit], NEG));
        p[young] = old;
        alive--;
        merges++;
    }
    return merges;
}
template <class Emit>
static inline long grid_elder_sweep(const float *f, const uint64_t *keys, long n_keys, int D, int H, int W,
                                    const GridOffsets &o, int negate, Emit emit) {
    return negate ? grid_elder_sweep_signed<true>(f, keys, n_keys, D, H, W, o, emit)
                  : grid_elder_sweep_signed<false>(f, keys, n_keys, D, H, W, o, emit);
}

// work(i) for every i in [0, n_items) over <= 16 threads (never sized by the machine's core count); thread 0 is the caller
template <class Work>
static inline void host_pool(int n_items, int n_threads, Work work) {
    int nt = n_threads < 1 ? 1 : (n_threads > 16 ? 16 : n_threads);
    if (nt > n_items) nt = n_items;
    auto run = [&](int t) {
        for (int i = t; i < n_items; i += nt) work(i);
    };
    if (nt <= 1) {
        run(0);
    } else {
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; t++) pool.emplace_back(run, t);
        run(0);
        for (auto &th : pool) th.join();
    }
}

}  // namespace mvd
