// H0 persistence (birth / death pairing) of a scalar field on a voxel grid -- SURVEY K12 / a-11.
//
// Replaces, for vertices + edges (maxdim 0), what the reference computes on the CPU through its vendored TopologyLayer
// C++ (nnunetv2/training/topologylayer/functional/persistence/): complex.cpp:136-146 (lower-star extension: a cell's
// value is the max of its vertex values, its critical vertex the arg-max), complex.cpp:182-196 (filtration order =
// sort by (value, dimension)), hom.cpp:51-69 (column reduction: restricted to vertices and edges it IS union-find with
// the elder rule), hom.cpp:155-185 (one bar per vertex, essential bars die at +inf).  The reference builds the boundary
// matrix in a std::map and reduces columns one by one; here
//   device: one key per grid edge = (order-preserving bits of max(g[u], g[v]))<<32 | edge index, all edges of the
//           D x H x W grid at once (k_grid_edge_keys), then ONE 64-bit radix sort (hipCUB / rocPRIM) = the filtration
//           order of the 1-cells; vertices need no sort: "older" is a comparison of (value, index);
//   host:   a single union-find sweep over the sorted edges with the elder rule (mvd_h0_pair_host) -- the inherently
//           sequential part, O(E alpha(V)) integer work on an 8 MB parent array.
// Integer / comparison work only: results are bit-exact against oracle/cc_oracle.c (same tie-breaking: vertices by
// (value, linear index), edges by (value, enumeration index)) and, as multisets of (birth, death), against the
// reference's own C++ (tests/golden/persistence_grid.json).
#include "persist_common.h"

#include <math.h>

using namespace mvd;

extern "C" {

long mvd_h0_num_edges(int D, int H, int W, int conn) {
    GridOffsets o;
    if (D <= 0 || H <= 0 || W <= 0 || grid_half_offsets(conn, &o)) return -1;
    return grid_valid_edges(D, H, W, o);
}

size_t mvd_h0_workspace_bytes(int D, int H, int W, int conn) {
    GridOffsets o;
    if (D <= 0 || H <= 0 || W <= 0 || grid_half_offsets(conn, &o)) return 0;
    const long total = (long)D * H * W * o.n;
    return (size_t)total * sizeof(uint64_t) + sort_u64_temp_bytes(total) + 512;
}

int mvd_h0_sorted_edges(const float *f, uint64_t *keys_sorted, int D, int H, int W, int conn, int sublevel, void *ws,
                        size_t ws_bytes, void *stream) {
    GridOffsets o;
    MVD_REQUIRE(f && keys_sorted && ws, "h0_sorted_edges: null pointer");
    MVD_REQUIRE(D > 0 && H > 0 && W > 0 && grid_half_offsets(conn, &o) == 0, "h0_sorted_edges: conn must be 6, 14 or 26");
    const long total = (long)D * H * W * o.n;
    MVD_REQUIRE(total < (1L << 31), "h0_sorted_edges: grid too large (edge index must fit 31 bits)");
    MVD_REQUIRE(ws_bytes >= mvd_h0_workspace_bytes(D, H, W, conn), "h0_sorted_edges: workspace too small");
    hipStream_t s = as_stream(stream);
    // super-level persistence = sub-level persistence of -f (nn/levelset.py:150-160)
    hipLaunchKernelGGL(k_grid_edge_keys, dim3(ew_blocks(total, 8192)), dim3(256), 0, s, f, reinterpret_cast<uint64_t *>(ws), D,
                       H, W, o, !sublevel);
    if (check_launch("h0_edge_keys")) return 1;
    hipError_t e = sort_u64_from_workspace(ws, ws_bytes, total, keys_sorted, s);
    if (e != hipSuccess) {
        set_error("h0_sorted_edges: radix sort: %s", hipGetErrorString(e));
        return 1;
    }
    return check_launch("h0_sort");
}

/* Host half (plain C++, no device access): elder-rule union-find over the sorted edge keys.
 * f_host: the field (as given, not sign-flipped); keys_host: the first n_edges = mvd_h0_num_edges() sorted keys.
 * death[v] = value at which the bar born at vertex v dies (+inf / -inf for the essential bar of each component under
 * sub-/super-level filtration, i.e. death = -(+inf) after undoing the sign flip), death_vertex[v] = critical (arg-max)
 * vertex of the killing edge or -1.  birth of the bar of vertex v is f_host[v].  Returns the number of essential bars,
 * < 0 for keys that are no sorted filtration of this grid. */
long mvd_h0_pair_host(const float *f_host, const uint64_t *keys_host, long n_edges, int D, int H, int W, int conn,
                      int sublevel, float *death, int64_t *death_vertex) {
    GridOffsets o;
    if (!f_host || !keys_host || !death || !death_vertex || D <= 0 || H <= 0 || W <= 0 || grid_half_offsets(conn, &o)) {
        set_error("h0_pair_host: bad arguments");
        return -1;
    }
    const long N = (long)D * H * W;
    if (N >= (1L << 31) || n_edges != grid_valid_edges(D, H, W, o)) {
        set_error("h0_pair_host: n_edges does not match the grid (%ld)", n_edges);
        return -1;
    }
    const float inf = sublevel ? INFINITY : -INFINITY;
    for (long i = 0; i < N; i++) {
        death[i] = inf;
        death_vertex[i] = -1;
    }
    const long rc = grid_elder_sweep(f_host, keys_host, n_edges, D, H, W, o, !sublevel,
                                         [&](int32_t young, int32_t crit, float val) {
                                             death[young] = sublevel ? val : -val;  // == ord2f(key >> 32), sign undone
                                             death_vertex[young] = crit;
                                         });
    if (rc < 0) {
        set_error("h0_pair_host: the keys are not a sorted filtration of the %dx%dx%d grid (or out of host memory)", W, H, D);
        return -1;
    }
    long ness = 0;
    for (long i = 0; i < N; i++) ness += isinf(death[i]) ? 1 : 0;
    return ness;
}
}
