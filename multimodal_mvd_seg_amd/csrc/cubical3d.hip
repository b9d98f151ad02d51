// 3-D cubical persistence (dimensions 0 and 2) of a batch of scalar fields, and the Wasserstein loss between such a
// diagram and the diagram of a binary mask -- the topological term of the dual-branch trainer (MVDTrainer.py:94-97,
// 907-925: CubicalComplex(dim=3) of the vessel logits and of the one-hot target, the features of dimension topo_feat_d = 2,
// WassersteinDistance; training/loss/TopoLoss.py is the same construction as a module, q = 2).
//
// Sublevel filtration of f [D,H,W] with voxels as closed top-dimensional cells.  Both dimensions built here are union-find:
//   dimension 0: the components of {f <= t} are 26-connected -> elder-rule H0 bars of the vertex / edge filtration on the
//                26-neighbourhood, edge value max(f[u], f[v]);
//   dimension 2: by Alexander duality a void of {f <= t} is a 6-connected component of {f > t} that does not reach the
//                outside of the grid -> elder-rule bars of the voxels in DESCENDING order on the 6-neighbourhood, edge value
//                min(f[u], f[v]), plus one outside vertex of value +inf joined to every border voxel (the one-voxel +inf
//                shell, never materialised: a border voxel gets ONE extra edge).  A component is born at its maximum d and
//                dies at the edge of value b that merges it into an older one: the bar (b, d).
//   Dimension 1 needs a boundary-matrix reduction and is not built.
//
//   device: k_grid_edge_keys -- one 64-bit key per (voxel, half-neighbour): ord(edge value of g) << 32 | (v * n_off + k)
//           with g = f (dimension 0) or -f (dimension 2), -0 folded to +0 -- and one 64-bit radix sort per sample (the
//           order of persist_common.h: vertices by (value, linear index), edges by (value, enumeration index));
//   host:   mvd_cub3d_pair_host, plain C++: one elder-rule union-find sweep per sample (grid_elder_sweep), samples over
//           <= 16 threads; the bars of non-zero length as (birth voxel, death voxel) rows;
//   device: the target's diagram is m copies of (0, 1): m is counted with mvd_cc_label and one border-flag pass;
//           the optimal matching of n bars to m identical points is a selection of the <= m bars of largest positive gain
//           (one stable descending radix sort of the fp64 gains per sample); the loss is reduced in fp64 in a fixed order;
//           the gradient is scattered by voxel-sorted runs (one thread owns a voxel's run): no float atomics anywhere.
#include "persist_common.h"

#include <math.h>

namespace mvd {

#define CUB3D_MAX_SAMPLES 4096
#define CUB3D_NO_KEY 0xffffffffu

// dimension 0: half of the 26-neighbourhood, f swept upwards; dimension 2: half of the 6-neighbourhood plus slot 3, the
// edge to the outside vertex, f swept downwards (negate = dim == 2)
static int cub3d_offsets(int dim, GridOffsets *o) {
    if (dim != 0 && dim != 2) return 1;
    grid_half_offsets(dim == 0 ? 26 : 6, o);
    if (dim == 2) {
        o->outside = o->n++;
        memset(o->off[o->outside], 0, sizeof(int) * 3);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------ the target's m
__global__ void k_cub3d_target_mask(const float *__restrict__ t, uint8_t *__restrict__ mask, long V, int dim) {
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x)
        mask[v] = dim == 2 ? (t[v] != 0.f) : (t[v] == 0.f);
}
// flags[root] = 1 for every component with a voxel on a face of the volume (every writer stores the same value)
__global__ void k_cub3d_border_flags(const int32_t *__restrict__ labels, int32_t *__restrict__ flags, int D, int H, int W) {
    const long V = (long)D * H * W;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        const int32_t l = labels[v];
        if (l <= 0 || l > V) continue;
        const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((long)W * H));
        if (x == 0 || x == W - 1 || y == 0 || y == H - 1 || z == 0 || z == D - 1) flags[l - 1] = 1;
    }
}
// m[0] += components whose canonical voxel (label == index + 1) carries no flag; integer atomics: exact
__global__ void k_cub3d_count_enclosed(const int32_t *__restrict__ labels, const int32_t *__restrict__ flags, long V,
                                       int32_t *__restrict__ m) {
    int32_t c = 0;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x)
        if (labels[v] == (int32_t)(v + 1) && flags[v] == 0) c++;
    if (c) atomicAdd(m, c);
}
__global__ void k_cub3d_minus_one(int32_t *__restrict__ m) {
    if (threadIdx.x == 0 && blockIdx.x == 0) m[0] = m[0] > 0 ? m[0] - 1 : 0;
}

// -------------------------------------------------------------------------------------------------- matching and loss
struct Cub3dBar {
    double b, d, c0, c1;
    bool ok;
};
__device__ inline int cub3d_sample_of(const int32_t *__restrict__ offsets, int N, long i) {
    int s = 0;
    while (s + 1 < N && i >= offsets[s + 1]) s++;
    return s;
}
__device__ inline Cub3dBar cub3d_bar(const float *__restrict__ field, const int32_t *__restrict__ bars, long i, int s, long V) {
    Cub3dBar r;
    const int32_t bv = bars[2 * i], dv = bars[2 * i + 1];
    r.ok = bv >= 0 && bv < V && dv >= 0 && dv < V;
    r.b = r.ok ? (double)field[(long)s * V + bv] : 0.0;
    r.d = r.ok ? (double)field[(long)s * V + dv] : 0.0;
    r.c0 = (r.d - r.b) * 0.5;                                   // L-inf distance to the diagonal
    r.c1 = fmax(fabs(r.b), fabs(1.0 - r.d));                     // L-inf distance to the point (0, 1)
    return r;
}
// monotone map of a double onto uint64; gains that are not strictly positive map to 0
__device__ inline uint64_t cub3d_gain_key(double g) {
    if (!(g > 0.0)) return 0ull;
    return (uint64_t)__double_as_longlong(g) | 0x8000000000000000ull;
}

__global__ void k_cub3d_gains(const float *__restrict__ field, const int32_t *__restrict__ bars,
                              const int32_t *__restrict__ offsets, int N, long V, long n_total, double q,
                              uint64_t *__restrict__ gkey, uint32_t *__restrict__ gidx) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_total) return;
    const int s = cub3d_sample_of(offsets, N, i);
    const Cub3dBar r = cub3d_bar(field, bars, i, s, V);
    const double gain = r.ok ? pow(r.c0, q) + pow(0.5, q) - pow(r.c1, q) : 0.0;
    gkey[i] = cub3d_gain_key(gain);
    gidx[i] = (uint32_t)i;
}

// sorted (descending, stable) gains of one sample: rank r < m with a positive gain is matched to a target point
__global__ void k_cub3d_select(const uint64_t *__restrict__ gkey_sorted, const uint32_t *__restrict__ gidx_sorted,
                               const int32_t *__restrict__ m, long n, uint8_t *__restrict__ selected) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    selected[gidx_sorted[r]] = (r < (long)m[0] && gkey_sorted[r] != 0ull) ? 1 : 0;
}

// one workgroup per sample: W^q = sum_unselected c0^q + sum_selected c1^q + (m - #selected) 2^-q, fp64, fixed order
__global__ void __launch_bounds__(1024) k_cub3d_wq(const float *__restrict__ field, const int32_t *__restrict__ bars,
                                                   const int32_t *__restrict__ offsets, const int32_t *__restrict__ m,
                                                   const uint8_t *__restrict__ selected, long V, double q,
                                                   double *__restrict__ wq) {
    __shared__ double sm[32];
    const int s = blockIdx.x;
    const long i0 = offsets[s], i1 = offsets[s + 1];
    double acc[2] = {0.0, 0.0};
    for (long i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        const Cub3dBar r = cub3d_bar(field, bars, i, s, V);
        if (!r.ok) continue;
        if (selected[i]) {
            acc[0] += pow(r.c1, q);
            acc[1] += 1.0;
        } else {
            acc[0] += pow(r.c0, q);
        }
    }
    block_sum<2>(acc, sm);
    if (threadIdx.x == 0) {
        const double rest = (double)m[s] - acc[1];
        wq[s] = acc[0] + (rest > 0.0 ? rest * pow(0.5, q) : 0.0);
    }
}
__global__ void k_cub3d_mean(const double *__restrict__ wq, int N, double q, float *__restrict__ out) {
    if (threadIdx.x || blockIdx.x) return;
    double s = 0.0;
    for (int i = 0; i < N; i++) s += wq[i] > 0.0 ? pow(wq[i], 1.0 / q) : 0.0;
    out[0] = (float)(s / (double)N);
}

// ----------------------------------------------------------------------------------------------------------- gradient
// entry e = 2 * bar + side (side 0: the birth coordinate, 1: the death coordinate) -> key = the global voxel it lands
// on, or CUB3D_NO_KEY for the coordinate of a selected bar that does not attain max(|b|, |1 - d|)
__global__ void k_cub3d_scatter_keys(const float *__restrict__ field, const int32_t *__restrict__ bars,
                                     const int32_t *__restrict__ offsets, const uint8_t *__restrict__ selected, int N, long V,
                                     long n_total, uint32_t *__restrict__ key, uint32_t *__restrict__ ent) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * n_total) return;
    const long i = e >> 1;
    const int side = (int)(e & 1);
    const int s = cub3d_sample_of(offsets, N, i);
    const int32_t vox = bars[2 * i + side];
    bool live = vox >= 0 && vox < V;
    if (live && selected && selected[i]) {
        const Cub3dBar r = cub3d_bar(field, bars, i, s, V);
        const bool death_takes = fabs(r.b) <= fabs(1.0 - r.d);  // at |b| == |1 - d| the death coordinate takes it
        live = r.ok && (side == 1) == death_takes;
    }
    key[e] = live ? (uint32_t)((long)s * V + vox) : CUB3D_NO_KEY;
    ent[e] = (uint32_t)e;
}

__device__ inline double cub3d_entry_grad(const float *__restrict__ field, const int32_t *__restrict__ bars,
                                          const int32_t *__restrict__ offsets, const uint8_t *__restrict__ selected,
                                          const double *__restrict__ wq, int N, long V, double q, uint32_t e) {
    const long i = e >> 1;
    const int side = (int)(e & 1);
    const int s = cub3d_sample_of(offsets, N, i);
    const double w = wq[s];
    if (!(w > 0.0)) return 0.0;
    const double scale = (1.0 / q) * pow(w, 1.0 / q - 1.0) / (double)N;
    const Cub3dBar r = cub3d_bar(field, bars, i, s, V);
    if (!selected[i]) {
        const double t = q * pow(r.c0, q - 1.0) * 0.5;
        return scale * (side ? t : -t);
    }
    if (r.c1 == 0.0) return 0.0;
    const double t = q * pow(r.c1, q - 1.0);
    if (side == 0) return scale * (r.b > 0.0 ? t : -t);          // d|b|/db
    return scale * (r.d > 1.0 ? t : -t);                         // d|1 - d|/dd
}

// one thread per sorted entry; the first entry of a voxel's run sums the run in sorted (= entry) order and stores it.
// gdiag != NULL: the diagram layer's backward, entry e receives gdiag[e]; else the loss's gradient times g_out[0].
__global__ void k_cub3d_scatter(const uint32_t *__restrict__ key, const uint32_t *__restrict__ ent, long n_ent,
                                const float *__restrict__ gdiag, const float *__restrict__ field,
                                const int32_t *__restrict__ bars, const int32_t *__restrict__ offsets,
                                const uint8_t *__restrict__ selected, const double *__restrict__ wq,
                                const float *__restrict__ g_out, int N, long V, double q, float *__restrict__ grad) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_ent) return;
    const uint32_t k = key[r];
    if (k == CUB3D_NO_KEY || (uint64_t)k >= (uint64_t)N * (uint64_t)V || (r > 0 && key[r - 1] == k)) return;
    double sum = 0.0;
    for (long j = r; j < n_ent && key[j] == k; j++) {
        const uint32_t e = ent[j];
        if ((long)e >= n_ent) continue;
        sum += gdiag ? (double)gdiag[e] : cub3d_entry_grad(field, bars, offsets, selected, wq, N, V, q, e);
    }
    grad[k] = gdiag ? (float)sum : (float)(sum * (double)g_out[0]);
}

static size_t cub3d_pairs_temp_u64(long n) {
    size_t t = 0;
    (void)hipcub::DeviceRadixSort::SortPairsDescending(nullptr, t, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                       (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0, 64);
    return t;
}
static size_t cub3d_pairs_temp_u32(long n) {
    size_t t = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0, 32);
    return t;
}

}  // namespace mvd

using namespace mvd;

extern "C" {

/* slots per sample of the key array (V * 13 for dimension 0, V * 4 for dimension 2); *n_valid = the keys that are edges
 * (the rest carry ~0 and sort last).  < 0: dim is neither 0 nor 2, or the grid is empty. */
long mvd_cub3d_num_keys(int D, int H, int W, int dim, long *n_valid) {
    GridOffsets o;
    if (D <= 0 || H <= 0 || W <= 0 || cub3d_offsets(dim, &o)) return -1;
    if (n_valid) *n_valid = grid_valid_edges(D, H, W, o);
    return (long)D * H * W * o.n;
}

size_t mvd_cub3d_workspace_bytes(int D, int H, int W, int dim) {
    GridOffsets o;
    if (D <= 0 || H <= 0 || W <= 0 || cub3d_offsets(dim, &o)) return 0;
    const long total = (long)D * H * W * o.n;
    if (total >= (1L << 31)) return 0;
    return sort_u64_workspace_bytes(total);
}

/* f [N][D][H][W] -> keys_sorted [N][num_keys], ascending per sample */
int mvd_cub3d_sorted_keys(const float *f, int N, int D, int H, int W, int dim, uint64_t *keys_sorted, void *ws,
                          size_t ws_bytes, void *stream) {
    GridOffsets o;
    MVD_REQUIRE(f && keys_sorted && ws, "cub3d_sorted_keys: null pointer");
    MVD_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "cub3d_sorted_keys: bad shape");
    MVD_REQUIRE(cub3d_offsets(dim, &o) == 0,
                "cub3d_sorted_keys: dimension %d is not built (0 and 2 are union-find; 1 needs a matrix reduction)", dim);
    const long V = (long)D * H * W, total = V * o.n;
    MVD_REQUIRE(total < (1L << 31), "cub3d_sorted_keys: grid too large (edge index must fit 31 bits)");
    const size_t need = mvd_cub3d_workspace_bytes(D, H, W, dim);
    MVD_REQUIRE(need && ws_bytes >= need, "cub3d_sorted_keys: workspace too small");
    hipStream_t s = as_stream(stream);
    for (int n = 0; n < N; n++) {  // the sorts share the unsorted keys and the temporary storage: stream order
        hipLaunchKernelGGL(k_grid_edge_keys, dim3(ew_blocks(total, 8192)), dim3(256), 0, s, f + (long)n * V,
                           reinterpret_cast<uint64_t *>(ws), D, H, W, o, dim == 2);
        if (check_launch("cub3d_keys")) return 1;
        hipError_t e = sort_u64_from_workspace(ws, ws_bytes, total, keys_sorted + (long)n * total, s);
        if (e != hipSuccess) {
            set_error("cub3d_sorted_keys: radix sort: %s", hipGetErrorString(e));
            return 1;
        }
    }
    return check_launch("cub3d_sort");
}

/* Host half (plain C++, no device access).  f_host [N][V]; keys_host [N][n_keys], the first n_keys = *n_valid sorted
 * keys of every sample.  bars [N][V][2] int32: rows (birth voxel, death voxel) of the bars with death > birth, in sweep
 * order, counts[n] of them in sample n.  Essential bars are dropped. */
int mvd_cub3d_pair_host(const float *f_host, const uint64_t *keys_host, long n_keys, int N, int D, int H, int W, int dim,
                        int32_t *bars, int32_t *counts, int n_threads) {
    GridOffsets o;
    MVD_REQUIRE(f_host && bars && counts && N > 0 && D > 0 && H > 0 && W > 0, "cub3d_pair_host: bad arguments");
    MVD_REQUIRE(cub3d_offsets(dim, &o) == 0,
                "cub3d_pair_host: dimension %d is not built (0 and 2 are union-find; 1 needs a matrix reduction)", dim);
    const long V = (long)D * H * W;
    MVD_REQUIRE(V * o.n < (1L << 31), "cub3d_pair_host: grid too large");
    MVD_REQUIRE(n_keys == grid_valid_edges(D, H, W, o) && (keys_host || n_keys == 0),
                "cub3d_pair_host: n_keys does not match the grid (%ld)", n_keys);
    const int negate = dim == 2;
    std::vector<long> rc((size_t)N, 0);
    host_pool(N, n_threads, [&](int n) {
        const float *f = f_host + (long)n * V;
        int32_t *rows = bars + (long)n * V * 2;
        long nb = 0;
        // the component of `young` is born at g[young] and dies at val = g[crit]: a bar of non-zero length iff val is
        // above; in f that is (young, crit) for dimension 0 and, the sweep running downwards, (crit, young) for dimension 2
        const long r = grid_elder_sweep(f, keys_host + (long)n * n_keys, n_keys, D, H, W, o, negate,
                                        [&](int32_t young, int32_t crit, float val) {
                                            if (!(val > fold_sign(f[young], negate))) return;
                                            rows[2 * nb] = negate ? crit : young;      // birth voxel
                                            rows[2 * nb + 1] = negate ? young : crit;  // death voxel
                                            nb++;
                                        });
        rc[n] = r < 0 ? -1 : nb;
    });
    for (int n = 0; n < N; n++) {
        MVD_REQUIRE(rc[n] >= 0, "cub3d_pair_host: the keys of sample %d are not a sorted filtration of the %dx%dx%d grid", n, W,
                    H, D);
        counts[n] = (int32_t)rc[n];
    }
    return 0;
}

size_t mvd_cub3d_target_workspace_bytes(int D, int H, int W) {
    if (D <= 0 || H <= 0 || W <= 0) return 0;
    const size_t V = (size_t)D * H * W;
    return al256(V) + al256(V * 4) + al256(V * 4 + 4) + 256;
}

/* target [N][D][H][W] fp32, binary.  m [N] int32 on the device: the number of points (0, 1) of the target's diagram --
 * dimension 2: the 6-connected foreground components that touch no face of the volume; dimension 0: the 26-connected
 * background components minus one, floored at 0. */
int mvd_cub3d_target_count(const float *target, int N, int D, int H, int W, int dim, int32_t *m, void *ws, size_t ws_bytes,
                           void *stream) {
    MVD_REQUIRE(target && m && ws && N > 0 && D > 0 && H > 0 && W > 0, "cub3d_target_count: bad arguments");
    MVD_REQUIRE(dim == 0 || dim == 2, "cub3d_target_count: dimension %d is not built", dim);
    const long V = (long)D * H * W;
    MVD_REQUIRE(V < 2147483647L, "cub3d_target_count: grid too large (int32 labels)");
    MVD_REQUIRE(ws_bytes >= mvd_cub3d_target_workspace_bytes(D, H, W), "cub3d_target_count: workspace too small");
    hipStream_t s = as_stream(stream);
    uint8_t *mask = reinterpret_cast<uint8_t *>(ws);
    int32_t *labels = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(ws) + al256((size_t)V));
    int32_t *flags = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(labels) + al256((size_t)V * 4));  // [V] + 1 scratch
    for (int n = 0; n < N; n++) {
        hipLaunchKernelGGL(k_cub3d_target_mask, dim3(ew_blocks(V, 8192)), dim3(256), 0, s, target + (long)n * V, mask, V, dim);
        if (check_launch("cub3d_target_mask")) return 1;
        if (dim == 0) {
            if (int rc = mvd_cc_label(mask, labels, m + n, D, H, W, 26, stream)) return rc;
            hipLaunchKernelGGL(k_cub3d_minus_one, dim3(1), dim3(64), 0, s, m + n);
        } else {
            if (int rc = mvd_cc_label(mask, labels, flags + V, D, H, W, 6, stream)) return rc;
            if (hipMemsetAsync(flags, 0, (size_t)V * 4, s) != hipSuccess || hipMemsetAsync(m + n, 0, 4, s) != hipSuccess) {
                set_error("cub3d_target_count: memset failed");
                return 1;
            }
            hipLaunchKernelGGL(k_cub3d_border_flags, dim3(ew_blocks(V, 8192)), dim3(256), 0, s, labels, flags, D, H, W);
            hipLaunchKernelGGL(k_cub3d_count_enclosed, dim3(ew_blocks(V, 8192)), dim3(256), 0, s, labels, flags, V, m + n);
        }
        if (check_launch("cub3d_target_count")) return 1;
    }
    return 0;
}

/* workspace of mvd_cub3d_match_fwd and mvd_cub3d_scatter_plan for n_total bars in all samples together */
size_t mvd_cub3d_match_workspace_bytes(long n_total) {
    if (n_total < 0 || 2 * n_total >= (1L << 31)) return 0;
    const long n = n_total < 1 ? 1 : n_total;
    const size_t a = 2 * al256((size_t)n * 8) + 2 * al256((size_t)n * 4) + cub3d_pairs_temp_u64(n);
    const size_t b = 2 * al256((size_t)n * 8) + cub3d_pairs_temp_u32(2 * n);
    return (a > b ? a : b) + 512;
}

/* field [N][V] fp32; bars [n_total][2] int32 (device), sample n owns rows [offsets[n], offsets[n+1]) -- offsets given on
 * the host AND on the device; m [N] int32 (device).  selected [n_total] uint8: 1 = matched to a target point;
 * wq [N] fp64: W^q per sample; out[0] = mean_n (W^q)^(1/q) in fp32. */
int mvd_cub3d_match_fwd(const float *field, const int32_t *bars, const int32_t *offsets_host, const int32_t *offsets_dev,
                        const int32_t *m, int N, long V, double q, uint8_t *selected, double *wq, float *out, void *ws,
                        size_t ws_bytes, void *stream) {
    MVD_REQUIRE(field && offsets_host && offsets_dev && m && wq && out && ws, "cub3d_match_fwd: null pointer");
    MVD_REQUIRE(N > 0 && N <= CUB3D_MAX_SAMPLES && V > 0 && (long)N * V < (1L << 32) - 1, "cub3d_match_fwd: bad shape");
    MVD_REQUIRE(q >= 1.0, "cub3d_match_fwd: q must be >= 1 (got %g)", q);
    MVD_REQUIRE(offsets_host[0] == 0, "cub3d_match_fwd: offsets must start at 0");
    for (int n = 0; n < N; n++) MVD_REQUIRE(offsets_host[n + 1] >= offsets_host[n], "cub3d_match_fwd: offsets must ascend");
    const long n_total = offsets_host[N];
    MVD_REQUIRE(n_total == 0 || (bars && selected), "cub3d_match_fwd: null pointer");
    const size_t need = mvd_cub3d_match_workspace_bytes(n_total);
    MVD_REQUIRE(need && ws_bytes >= need, "cub3d_match_fwd: workspace too small");
    hipStream_t s = as_stream(stream);
    if (n_total > 0) {
        char *p = reinterpret_cast<char *>(ws);
        uint64_t *gkey = reinterpret_cast<uint64_t *>(p);
        p += al256((size_t)n_total * 8);
        uint64_t *gkey_s = reinterpret_cast<uint64_t *>(p);
        p += al256((size_t)n_total * 8);
        uint32_t *gidx = reinterpret_cast<uint32_t *>(p);
        p += al256((size_t)n_total * 4);
        uint32_t *gidx_s = reinterpret_cast<uint32_t *>(p);
        p += al256((size_t)n_total * 4);
        const size_t temp_cap = ws_bytes - (size_t)(p - reinterpret_cast<char *>(ws));
        hipLaunchKernelGGL(k_cub3d_gains, dim3(cdiv(n_total, 256)), dim3(256), 0, s, field, bars, offsets_dev, N, V, n_total, q,
                           gkey, gidx);
        if (check_launch("cub3d_gains")) return 1;
        for (int n = 0; n < N; n++) {
            const long i0 = offsets_host[n], cnt = offsets_host[n + 1] - i0;
            if (cnt == 0) continue;
            size_t temp_bytes = temp_cap;
            // stable: equal gains keep the order of the bar index
            hipError_t e = hipcub::DeviceRadixSort::SortPairsDescending(p, temp_bytes, gkey + i0, gkey_s + i0, gidx + i0,
                                                                        gidx_s + i0, (int)cnt, 0, 64, s);
            if (e != hipSuccess) {
                set_error("cub3d_match_fwd: radix sort: %s", hipGetErrorString(e));
                return 1;
            }
            hipLaunchKernelGGL(k_cub3d_select, dim3(cdiv(cnt, 256)), dim3(256), 0, s, gkey_s + i0, gidx_s + i0, m + n, cnt,
                               selected);
        }
        if (check_launch("cub3d_select")) return 1;
    }
    hipLaunchKernelGGL(k_cub3d_wq, dim3(N), dim3(1024), 0, s, field, bars, offsets_dev, m, selected, V, q, wq);
    hipLaunchKernelGGL(k_cub3d_mean, dim3(1), dim3(64), 0, s, wq, N, q, out);
    return check_launch("cub3d_wq");
}

/* The order in which the gradient entries (2 per bar: birth, death coordinate) reach the voxels: key_sorted / order
 * [2 n_total] uint32.  selected == NULL: every entry is live (the diagram layer); else the entries of the loss. */
int mvd_cub3d_scatter_plan(const float *field, const int32_t *bars, const int32_t *offsets_dev, const uint8_t *selected, int N,
                           long V, long n_total, uint32_t *key_sorted, uint32_t *order, void *ws, size_t ws_bytes,
                           void *stream) {
    MVD_REQUIRE(field && bars && offsets_dev && key_sorted && order && ws, "cub3d_scatter_plan: null pointer");
    MVD_REQUIRE(N > 0 && N <= CUB3D_MAX_SAMPLES && V > 0 && (long)N * V < (1L << 32) - 1 && n_total > 0,
                "cub3d_scatter_plan: bad shape");
    const size_t need = mvd_cub3d_match_workspace_bytes(n_total);
    MVD_REQUIRE(need && ws_bytes >= need, "cub3d_scatter_plan: workspace too small");
    hipStream_t s = as_stream(stream);
    char *p = reinterpret_cast<char *>(ws);
    uint32_t *key = reinterpret_cast<uint32_t *>(p);
    p += al256((size_t)n_total * 8);
    uint32_t *ent = reinterpret_cast<uint32_t *>(p);
    p += al256((size_t)n_total * 8);
    size_t temp_bytes = ws_bytes - (size_t)(p - reinterpret_cast<char *>(ws));
    hipLaunchKernelGGL(k_cub3d_scatter_keys, dim3(cdiv(2 * n_total, 256)), dim3(256), 0, s, field, bars, offsets_dev, selected, N,
                       V, n_total, key, ent);
    if (check_launch("cub3d_scatter_keys")) return 1;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(p, temp_bytes, key, key_sorted, ent, order, (int)(2 * n_total), 0, 32, s);
    if (e != hipSuccess) {
        set_error("cub3d_scatter_plan: radix sort: %s", hipGetErrorString(e));
        return 1;
    }
    return check_launch("cub3d_scatter_plan");
}

/* grad [N][V] = g_out[0] * d out / d field: zeroed, then ONE launch; every voxel's run summed in a fixed order */
int mvd_cub3d_match_bwd(const float *field, const int32_t *bars, const int32_t *offsets_dev, const uint8_t *selected,
                        const double *wq, const float *g_out, const uint32_t *key_sorted, const uint32_t *order, int N, long V,
                        long n_total, double q, float *grad, void *stream) {
    MVD_REQUIRE(field && offsets_dev && wq && g_out && grad, "cub3d_match_bwd: null pointer");
    MVD_REQUIRE(N > 0 && N <= CUB3D_MAX_SAMPLES && V > 0 && (long)N * V < (1L << 32) - 1 && n_total >= 0 && q >= 1.0,
                "cub3d_match_bwd: bad arguments");
    MVD_REQUIRE(n_total == 0 || (bars && selected && key_sorted && order), "cub3d_match_bwd: null pointer");
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(grad, 0, sizeof(float) * (size_t)N * (size_t)V, s) != hipSuccess) {
        set_error("cub3d_match_bwd: memset failed");
        return 1;
    }
    if (n_total == 0) return 0;
    hipLaunchKernelGGL(k_cub3d_scatter, dim3(cdiv(2 * n_total, 256)), dim3(256), 0, s, key_sorted, order, 2 * n_total,
                       (const float *)nullptr, field, bars, offsets_dev, selected, wq, g_out, N, V, q, grad);
    return check_launch("cub3d_match_bwd");
}

/* grad [N][V] = the diagram gradient g_diag [n_total][2] added onto the bars' voxels (plan made with selected == NULL) */
int mvd_cub3d_diagram_bwd(const float *g_diag, const uint32_t *key_sorted, const uint32_t *order, int N, long V, long n_total,
                          float *grad, void *stream) {
    MVD_REQUIRE(grad && N > 0 && V > 0 && (long)N * V < (1L << 32) - 1 && n_total >= 0, "cub3d_diagram_bwd: bad arguments");
    MVD_REQUIRE(n_total == 0 || (g_diag && key_sorted && order), "cub3d_diagram_bwd: null pointer");
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(grad, 0, sizeof(float) * (size_t)N * (size_t)V, s) != hipSuccess) {
        set_error("cub3d_diagram_bwd: memset failed");
        return 1;
    }
    if (n_total == 0) return 0;
    hipLaunchKernelGGL(k_cub3d_scatter, dim3(cdiv(2 * n_total, 256)), dim3(256), 0, s, key_sorted, order, 2 * n_total, g_diag,
                       (const float *)nullptr, (const int32_t *)nullptr, (const int32_t *)nullptr, (const uint8_t *)nullptr,
                       (const double *)nullptr, (const float *)nullptr, N, V, 0.0, grad);
    return check_launch("cub3d_diagram_bwd");
}
}
