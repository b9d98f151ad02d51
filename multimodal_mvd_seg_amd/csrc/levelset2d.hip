// Level-set persistence (dimensions 0 and 1) of a batch of 2-D images on the Freudenthal triangulation, and the
// persistence topological loss built on it.
//
// Replaces what the reference computes per sample and class on the CPU: nn/levelset.py:64-93,137-163 (LevelSetLayer2D on
// init_freudenthal_2d), complex.cpp:136-146 (lower-star extension), complex.cpp:182-196 (filtration order), hom.cpp (the
// column reduction), nn/features.py:128-150 (TopKBarcodeLengths), loss/Topo_Loss.py:16-85 (TopoLoss) and cohom.cpp:148-196
// (persistence_backward).
//
// Complex of one [H, W] plane (width = W): V = H*W vertices in row-major order; E = H(W-1) + (H-1)W + (H-1)(W-1) edges --
// horizontal, vertical, then the diagonal (ind, ind+W+1) of every square; T = 2(H-1)(W-1) triangles, (ind, ind+1, ind+W+1)
// and (ind, ind+W, ind+W+1) of every square.  Indices within a dimension follow that order.  Lower-star filtration of
// g = f (sublevel) or -f (super-level, -0 folded to +0); total order (value, dimension, index).
//
//   device: k_ls2d_keys writes key = ord(value) << 32 | dimension << 30 | index of every cell of all P problems (problem p
//           = plane (b, channels[j]) of a [B, C, H, W] tensor, p = b * n_channels + j, read in place), then one merge sort
//           per problem segment, in place (block sorts + merge-path passes: no workgroup ever waits on another one, which
//           the look-back of the one-sweep radix sort would; a segmented radix sort keeps one workgroup per segment and was
//           8 to 16 times slower at 128^2 .. 256^2) = P filtration orders.
//   host:   mvd_ls2d_pair_host, plain C++: per problem a forward elder-rule union-find over vertices + edges (dimension 0)
//           and a BACKWARD elder-rule union-find over the dual graph (triangles + one outer face, joined by the edges) for
//           dimension 1 -- on a triangulated disc that is the whole reduction.  Problems are spread over <= 16 threads.
//   device: top-k bar lengths, the fused loss (fp64, fixed order), its gradient and the diagram gradient: every sum runs
//           in a fixed order, without float atomics.
// Comparison / integer work up to the lengths; each length is one fp32 subtraction.
#include "persist_common.h"

#include <math.h>

namespace mvd {

#define LS2D_MAX_CH 32
#define LS2D_MAX_K 64
#define LS2D_IDX_MASK 0x3fffffffu

struct Ls2dChannels {
    int n;
    int ch[LS2D_MAX_CH];
};

struct Ls2dGeom {
    int H, W;
    long V, Eh, Ev, Ed, E, T, n;  // n = cells in the sort: V + E (+ T when maxdim >= 1)
};

__host__ __device__ inline Ls2dGeom ls2d_geom(int H, int W, int maxdim) {
    Ls2dGeom g;
    g.H = H;
    g.W = W;
    g.V = (long)H * W;
    g.Eh = (long)H * (W - 1);
    g.Ev = (long)(H - 1) * W;
    g.Ed = (long)(H - 1) * (W - 1);
    g.E = g.Eh + g.Ev + g.Ed;
    g.T = maxdim >= 1 ? 2 * g.Ed : 0;
    g.n = g.V + g.E + g.T;
    return g;
}

// the two vertices of edge e (u < v)
__host__ __device__ inline void ls2d_edge_vertices(const Ls2dGeom &g, long e, long *u, long *v) {
    if (e < g.Eh) {
        const long i = e / (g.W - 1), j = e - i * (g.W - 1);
        *u = i * g.W + j;
        *v = *u + 1;
    } else if (e < g.Eh + g.Ev) {
        *u = e - g.Eh;
        *v = *u + g.W;
    } else {
        const long s = e - g.Eh - g.Ev, i = s / (g.W - 1), j = s - i * (g.W - 1);
        *u = i * g.W + j;
        *v = *u + g.W + 1;
    }
}
// the three vertices of triangle t (a < b < c)
__host__ __device__ inline void ls2d_tri_vertices(const Ls2dGeom &g, long t, long *a, long *b, long *c) {
    const long s = t >> 1, i = s / (g.W - 1), j = s - i * (g.W - 1);
    *a = i * g.W + j;
    *b = (t & 1) ? *a + g.W : *a + 1;
    *c = *a + g.W + 1;
}

struct Ls2dKeyLess {
    __host__ __device__ bool operator()(const uint64_t &a, const uint64_t &b) const { return a < b; }
};

// one thread per (problem, cell)
__global__ void k_ls2d_keys(const float *__restrict__ x, uint64_t *__restrict__ keys, int B, int C, const Ls2dChannels chs,
                            const Ls2dGeom g, int sublevel) {
    const long P = (long)B * chs.n, total = P * g.n;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const long p = q / g.n, c = q - p * g.n;
        const int b = (int)(p / chs.n), j = (int)(p - (long)b * chs.n);
        const float *f = x + ((long)b * C + chs.ch[j]) * g.V;
        float val;
        uint32_t lo;
        if (c < g.V) {
            val = fold_sign(f[c], !sublevel);
            lo = (uint32_t)c;
        } else if (c < g.V + g.E) {
            long u, v;
            ls2d_edge_vertices(g, c - g.V, &u, &v);
            const float a = fold_sign(f[u], !sublevel), d = fold_sign(f[v], !sublevel);
            val = a < d ? d : a;
            lo = (1u << 30) | (uint32_t)(c - g.V);
        } else {
            long u, v, w;
            ls2d_tri_vertices(g, c - g.V - g.E, &u, &v, &w);
            const float a = fold_sign(f[u], !sublevel), d = fold_sign(f[v], !sublevel), e = fold_sign(f[w], !sublevel);
            val = a < d ? d : a;
            val = val < e ? e : val;
            lo = (2u << 30) | (uint32_t)(c - g.V - g.E);
        }
        keys[q] = ((uint64_t)f2ord(val) << 32) | lo;
    }
}

// ------------------------------------------------------------------------------------------------------------ host pairing
// bars row r of one problem: {bits of the birth value, bits of the death value, birth critical vertex, death critical vertex}
static inline void ls2d_put(int32_t *row, float birth, float death, int32_t bv, int32_t dv) {
    memcpy(row, &birth, 4);
    memcpy(row + 1, &death, 4);
    row[2] = bv;
    row[3] = dv;
}

static int ls2d_pair_one(const uint64_t *keys, const Ls2dGeom &g, int sublevel, int32_t *bars, int32_t *edge_row) {
    const long V = g.V, E = g.E, T = g.T, n = g.n;
    std::vector<float> gv((size_t)V), tval((size_t)T);
    std::vector<int32_t> rank((size_t)V), par((size_t)(V > T + 1 ? V : T + 1)), tpos((size_t)T + 1);
    const float sgn = sublevel ? 1.f : -1.f;
    const float inf = sublevel ? INFINITY : -INFINITY;
    long seen[3] = {0, 0, 0};
    // dimension 0: forward sweep, the component founded later (larger position in the order) dies
    for (long i = 0; i < n; i++) {
        const uint32_t lo = (uint32_t)keys[i], dim = lo >> 30, idx = lo & LS2D_IDX_MASK;
        const float val = ord2f((uint32_t)(keys[i] >> 32));
        if (dim > 2 || (i > 0 && keys[i] < keys[i - 1])) return 1;
        if ((dim == 0 && idx >= V) || (dim == 1 && idx >= E) || (dim == 2 && idx >= T)) return 1;
        seen[dim]++;
        if (dim == 0) {
            gv[idx] = val;
            rank[idx] = (int32_t)i;
            par[idx] = (int32_t)idx;
            ls2d_put(bars + 4 * (long)idx, sgn * val, inf, (int32_t)idx, -1);
        } else if (dim == 1) {
            long u, v;
            ls2d_edge_vertices(g, idx, &u, &v);
            const int32_t a = uf_find(par.data(), (int32_t)u), b = uf_find(par.data(), (int32_t)v);
            if (a == b) {
                edge_row[idx] = -1;  // opens a 1-cycle: paired in the backward sweep
                continue;
            }
            const int32_t young = rank[a] > rank[b] ? a : b, old = young == a ? b : a;
            int32_t *row = bars + 4 * (long)young;
            const float d = sgn * val;
            memcpy(row + 1, &d, 4);
            row[3] = (int32_t)(gv[u] >= gv[v] ? u : v);  // first maximal vertex (complex.cpp:142)
            edge_row[idx] = young;
            par[young] = old;
        } else {
            tval[idx] = val;
        }
    }
    if (seen[0] != V || seen[1] != E || seen[2] != T) return 1;
    if (T == 0) return 0;
    // dimension 1: backward sweep over the dual graph; node T is the outer face, the eldest of all
    const int32_t outer = (int32_t)T;
    par[outer] = outer;
    tpos[outer] = INT32_MAX;
    const long W1 = g.W - 1;
    for (long i = n - 1; i >= 0; i--) {
        const uint32_t lo = (uint32_t)keys[i], dim = lo >> 30, idx = lo & LS2D_IDX_MASK;
        if (dim == 2) {
            par[idx] = (int32_t)idx;
            tpos[idx] = (int32_t)i;
        } else if (dim == 1 && edge_row[idx] < 0) {
            int32_t t1, t2;
            if ((long)idx < g.Eh) {  // horizontal: lower triangle of the square above, upper triangle of the square below
                const long r = idx / W1, c = idx - r * W1;
                t1 = r > 0 ? (int32_t)(2 * ((r - 1) * W1 + c) + 1) : outer;
                t2 = r < g.H - 1 ? (int32_t)(2 * (r * W1 + c)) : outer;
            } else if ((long)idx < g.Eh + g.Ev) {  // vertical: upper triangle of the left square, lower of the right one
                const long q = idx - g.Eh, r = q / g.W, c = q - r * g.W;
                t1 = c > 0 ? (int32_t)(2 * (r * W1 + c - 1)) : outer;
                t2 = c < W1 ? (int32_t)(2 * (r * W1 + c) + 1) : outer;
            } else {
                const long s = idx - g.Eh - g.Ev;
                t1 = (int32_t)(2 * s);
                t2 = (int32_t)(2 * s + 1);
            }
            const int32_t a = uf_find(par.data(), t1), b = uf_find(par.data(), t2);
            if (a == b) return 1;  // a positive edge always separates two dual components
            const int32_t dying = tpos[a] < tpos[b] ? a : b, keep = dying == a ? b : a;
            long u, v, x, y, z;
            ls2d_edge_vertices(g, idx, &u, &v);
            ls2d_tri_vertices(g, dying, &x, &y, &z);
            const int32_t bv = (int32_t)(gv[u] >= gv[v] ? u : v);
            const int32_t dv = (int32_t)((gv[x] >= gv[y] && gv[x] >= gv[z]) ? x : (gv[y] >= gv[z] ? y : z));
            ls2d_put(bars + 4 * (V + dying), sgn * ord2f((uint32_t)(keys[i] >> 32)), sgn * tval[dying], bv, dv);
            edge_row[idx] = (int32_t)(V + dying);
            par[dying] = keep;
        }
    }
    for (long e = 0; e < E; e++)
        if (edge_row[e] < 0) return 1;
    return 0;
}

// ----------------------------------------------------------------------------------------------------------------- top-k
__device__ inline float ls2d_length(const int4 row, int sublevel) {
    const float b = __int_as_float(row.x), d = __int_as_float(row.y);
    const float len = sublevel ? d - b : b - d;  // end - start of get_start_end (features.py:6-21)
    return (len < INFINITY && len > 0.f) ? len : 0.f;  // infinite and NaN lengths -> 0 (features.py:41-42)
}

// one workgroup per (problem, dimension): k rounds of "largest key below the previous one", key = length bits << 32 | ~row
__global__ void __launch_bounds__(1024) k_ls2d_topk(const int32_t *__restrict__ bars, long V, long T, int sublevel, int k,
                                                    float *__restrict__ lengths, int32_t *__restrict__ index) {
    const int p = blockIdx.x >> 1, dim = blockIdx.x & 1;
    const long rows = V + T, r0 = dim ? V : 0, r1 = dim ? V + T : V;
    const int4 *pb = reinterpret_cast<const int4 *>(bars) + (long)p * rows;  // one 16-byte row per load
    float *out_l = lengths + ((long)p * 2 + dim) * k;
    int32_t *out_i = index + ((long)p * 2 + dim) * k;
    __shared__ uint64_t red[16];
    __shared__ uint64_t best;
    uint64_t prev = ~0ull;
    for (int round = 0; round < k; round++) {
        uint64_t m = 0;
#pragma unroll 4
        for (long r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
            const float len = ls2d_length(pb[r], sublevel);
            const uint64_t key = ((uint64_t)__float_as_uint(len) << 32) | (uint32_t)~(uint32_t)r;
            if (key < prev && key > m) m = key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t t = __shfl_down(m, o, 64);
            m = t > m ? t : m;
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t b = 0;
            for (int w = 0; w < (int)((blockDim.x + 63) >> 6); w++) b = red[w] > b ? red[w] : b;
            best = b;
        }
        __syncthreads();
        prev = best;
        const uint32_t bits = (uint32_t)(prev >> 32);
        if (bits == 0) {  // only zero-length bars (or none) are left: zero padding (pad_k, features.py:113-125)
            for (int j = round + threadIdx.x; j < k; j += blockDim.x) {
                out_l[j] = 0.f;
                out_i[j] = -1;
            }
            break;
        }
        if (threadIdx.x == 0) {
            out_l[round] = __uint_as_float(bits);
            out_i[round] = (int32_t)~(uint32_t)prev;
        }
        __syncthreads();
    }
}

// d lengths -> d diagram: bar `index` of (p, dim) receives +g on its end column and -g on its start column
__global__ void k_ls2d_topk_bwd(const float *__restrict__ g, const int32_t *__restrict__ index, long V, long T, int sublevel,
                                int k, long total, float *__restrict__ gbars /* [P][V+T][2], zeroed */) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const long p = q / (2 * k);
    const int32_t row = index[q];
    if (row < 0) return;
    float *o = gbars + ((long)p * (V + T) + row) * 2;
    o[0] = sublevel ? -g[q] : g[q];
    o[1] = sublevel ? g[q] : -g[q];
}

// --------------------------------------------------------------------------------------------------------- loss and gradient
__device__ inline int ls2d_beta(const int32_t *label, int b, int n_label, int cls, int dim) {
    const int v = label[((long)b * n_label + cls) * 2 + dim];
    return v < 0 ? 0 : v;
}

// out[0] = (1 / B) sum_p sum_dim sum_j sign(j < beta) * len^2 in fp64, fixed order (one workgroup)
__global__ void __launch_bounds__(256) k_ls2d_topoloss_fwd(const float *__restrict__ lengths, const int32_t *__restrict__ label,
                                                           int B, const Ls2dChannels idx, int n_label, int k,
                                                           float *__restrict__ out) {
    __shared__ double sm[16];
    const long total = (long)B * idx.n * 2 * k;
    double acc[1] = {0.0};
    for (long q = threadIdx.x; q < total; q += blockDim.x) {
        const int j = (int)(q % k), dim = (int)((q / k) & 1);
        const long p = q / (2 * k);
        const int b = (int)(p / idx.n), c = idx.ch[p - (long)b * idx.n];
        const double len = (double)lengths[q];
        acc[0] += (j < ls2d_beta(label, b, n_label, c, dim) ? -1.0 : 1.0) * len * len;
    }
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) out[0] = (float)(acc[0] / (double)B);
}

// one workgroup per problem, one thread per (dimension, bar, endpoint): contribution (g / B) * sign * (2 len), positive on
// the end of the bar and negative on its start; the first thread that names a vertex sums all contributions to it in
// thread order and stores the sum
__global__ void __launch_bounds__(4 * LS2D_MAX_K) k_ls2d_topoloss_bwd(
    const float *__restrict__ lengths, const int32_t *__restrict__ index, const int32_t *__restrict__ bars,
    const int32_t *__restrict__ label, const float *__restrict__ gout, int B, int C, const Ls2dChannels idx, int n_label,
    int k, long V, long T, int sublevel, float *__restrict__ grad) {
    __shared__ int32_t tgt[4 * LS2D_MAX_K];
    __shared__ float con[4 * LS2D_MAX_K];
    const int p = blockIdx.x, e = threadIdx.x, ne = 4 * k;
    const int b = p / idx.n, c = idx.ch[p - b * idx.n];
    int32_t target = -1;
    float contrib = 0.f;
    if (e < ne) {
        const int dim = e / (2 * k), j = (e >> 1) % k, side = e & 1;
        const long q = ((long)p * 2 + dim) * k + j;
        const int32_t row = index[q];
        if (row >= 0) {
            const float gs = gout[0] / (float)B;
            const float sign = j < ls2d_beta(label, b, n_label, c, dim) ? -1.f : 1.f;
            const float v = (gs * sign) * (2.f * lengths[q]);
            const bool is_end = sublevel ? side == 1 : side == 0;
            contrib = is_end ? v : -v;
            target = bars[((long)p * (V + T) + row) * 4 + 2 + side];
        }
        tgt[e] = target;
        con[e] = contrib;
    }
    __syncthreads();
    if (e >= ne || target < 0) return;
    for (int i = 0; i < e; i++)
        if (tgt[i] == target) return;
    float s = contrib;
    for (int i = e + 1; i < ne; i++)
        if (tgt[i] == target) s += con[i];
    grad[((long)b * C + (c + 1)) * V + target] = s;
}

// persistence_backward (cohom.cpp:148-196) as a gather: vertex v collects the gradient of its own birth, then of the <= 6
// incident edges and <= 6 incident triangles whose critical vertex it is, in enumeration order
__global__ void k_ls2d_diagram_bwd(const float *__restrict__ g0, const float *__restrict__ g1, const int32_t *__restrict__ bars,
                                   const int32_t *__restrict__ edge_row, int B, int C, const Ls2dChannels chs,
                                   const Ls2dGeom g, float *__restrict__ grad) {
    const long P = (long)B * chs.n, total = P * g.V;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const long p = q / g.V, v = q - p * g.V;
    const int b = (int)(p / chs.n), j = (int)(p - (long)b * chs.n);
    const int r = (int)(v / g.W), c = (int)(v - (long)r * g.W), H = g.H, W = g.W;
    const long W1 = W - 1;
    const int32_t *pb = bars + p * (g.V + g.T) * 4;
    const int32_t *er = edge_row + p * g.E;
    const float *q0 = g0 + p * g.V * 2, *q1 = g1 ? g1 + p * g.T * 2 : nullptr;
    float s = q0[2 * v];
    long ed[6];
    ed[0] = c > 0 ? (long)r * W1 + c - 1 : -1;
    ed[1] = c < W1 ? (long)r * W1 + c : -1;
    ed[2] = r > 0 ? g.Eh + (long)(r - 1) * W + c : -1;
    ed[3] = r < H - 1 ? g.Eh + (long)r * W + c : -1;
    ed[4] = (r > 0 && c > 0) ? g.Eh + g.Ev + (long)(r - 1) * W1 + c - 1 : -1;
    ed[5] = (r < H - 1 && c < W1) ? g.Eh + g.Ev + (long)r * W1 + c : -1;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        if (ed[i] < 0) continue;
        const int32_t row = er[ed[i]];
        if (row < 0) continue;  // maxdim 0: an edge that opens a 1-cycle is no endpoint of a returned bar
        if (row < g.V) {
            if (pb[4 * (long)row + 3] == (int32_t)v) s += q0[2 * (long)row + 1];
        } else if (q1 && pb[4 * (long)row + 2] == (int32_t)v) {
            s += q1[2 * ((long)row - g.V)];
        }
    }
    if (q1 && g.T > 0) {
        long tr[6];
        const bool up = r > 0, dn = r < H - 1, lf = c > 0, rt = c < W1;
        tr[0] = (up && lf) ? 2 * ((long)(r - 1) * W1 + c - 1) : -1;
        tr[1] = (up && lf) ? 2 * ((long)(r - 1) * W1 + c - 1) + 1 : -1;
        tr[2] = (up && rt) ? 2 * ((long)(r - 1) * W1 + c) + 1 : -1;
        tr[3] = (dn && lf) ? 2 * ((long)r * W1 + c - 1) : -1;
        tr[4] = (dn && rt) ? 2 * ((long)r * W1 + c) : -1;
        tr[5] = (dn && rt) ? 2 * ((long)r * W1 + c) + 1 : -1;
#pragma unroll
        for (int i = 0; i < 6; i++)
            if (tr[i] >= 0 && pb[4 * (g.V + tr[i]) + 3] == (int32_t)v) s += q1[2 * tr[i] + 1];
    }
    grad[((long)b * C + chs.ch[j]) * g.V + v] = s;
}

// counts[p] = {bars of non-zero length in dimension 0 -- the essential bar counted iff it is born above the floor 0 --,
// bars of non-zero length in dimension 1}
__global__ void __launch_bounds__(1024) k_ls2d_count(const int32_t *__restrict__ bars, long V, long T, int sublevel,
                                                    int32_t *__restrict__ counts) {
    __shared__ double sm[32];
    const int4 *pb = reinterpret_cast<const int4 *>(bars) + (long)blockIdx.x * (V + T);
    double acc[2] = {0.0, 0.0};
#pragma unroll 4
    for (long r = threadIdx.x; r < V + T; r += blockDim.x) {
        const int4 row = pb[r];
        const float bth = __int_as_float(row.x), dth = __int_as_float(row.y);
        const bool nz = row.w < 0 ? bth != 0.f : bth != dth;
        if (nz) acc[r < V ? 0 : 1] += 1.0;
    }
    block_sum<2>(acc, sm);
    if (threadIdx.x == 0) {
        counts[2 * blockIdx.x] = (int32_t)acc[0];
        counts[2 * blockIdx.x + 1] = (int32_t)acc[1];
    }
}

// planes[b][c][i] = (label[b][i] == c) as 0 / 1 floats
__global__ void k_ls2d_onehot(const float *__restrict__ label, float *__restrict__ planes, int B, int C, long V) {
    const long total = (long)B * C * V;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const long i = q % V, bc = q / V;
        const int c = (int)(bc % C);
        planes[q] = label[(bc / C) * V + i] == (float)c ? 1.f : 0.f;
    }
}

static int ls2d_channels(const int *channels, int n, int C, Ls2dChannels *out, const char *what) {
    if (!channels || n < 1 || n > LS2D_MAX_CH) {
        set_error("%s: 1..%d channels", what, LS2D_MAX_CH);
        return 1;
    }
    out->n = n;
    for (int i = 0; i < n; i++) {
        if (channels[i] < 0 || channels[i] >= C) {
            set_error("%s: channel %d outside [0, %d)", what, channels[i], C);
            return 1;
        }
        for (int j = 0; j < i; j++)
            if (channels[j] == channels[i]) {
                set_error("%s: channel %d listed twice", what, channels[i]);
                return 1;
            }
        out->ch[i] = channels[i];
    }
    return 0;
}

}  // namespace mvd

using namespace mvd;

extern "C" {

long mvd_ls2d_num_cells(int H, int W, int maxdim, long *nv, long *ne, long *nt) {
    if (H <= 0 || W <= 0 || maxdim < 0 || maxdim > 1) return -1;
    const Ls2dGeom g = ls2d_geom(H, W, maxdim);
    if (nv) *nv = g.V;
    if (ne) *ne = g.E;
    if (nt) *nt = g.T;
    return g.n;
}

size_t mvd_ls2d_workspace_bytes(int P, int H, int W, int maxdim) {
    if (P <= 0 || H <= 0 || W <= 0 || maxdim < 0 || maxdim > 1) return 0;
    const Ls2dGeom g = ls2d_geom(H, W, maxdim);
    if ((long)P * g.n >= (1L << 31)) return 0;
    size_t temp = 0;
    (void)hipcub::DeviceMergeSort::SortKeys(nullptr, temp, (uint64_t *)nullptr, (int)g.n, Ls2dKeyLess());
    return temp + 512;
}

int mvd_ls2d_sorted_keys(const float *x, int B, int C, int H, int W, const int *channels, int n_channels, int sublevel,
                         int maxdim, uint64_t *keys_sorted, void *ws, size_t ws_bytes, void *stream) {
    Ls2dChannels chs;
    MVD_REQUIRE(x && keys_sorted && ws, "ls2d_sorted_keys: null pointer");
    MVD_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && maxdim >= 0 && maxdim <= 1, "ls2d_sorted_keys: bad shape or maxdim");
    if (ls2d_channels(channels, n_channels, C, &chs, "ls2d_sorted_keys")) return 2;
    const Ls2dGeom g = ls2d_geom(H, W, maxdim);
    const int P = B * n_channels;
    const long total = (long)P * g.n;
    MVD_REQUIRE(g.E + g.T < (1L << 30) && total < (1L << 31), "ls2d_sorted_keys: too many cells (index must fit 30 bits)");
    const size_t need = mvd_ls2d_workspace_bytes(P, H, W, maxdim);
    MVD_REQUIRE(need && ws_bytes >= need, "ls2d_sorted_keys: workspace too small");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_ls2d_keys, dim3(ew_blocks(total, 8192)), dim3(256), 0, s, x, keys_sorted, B, C, chs, g, sublevel);
    if (check_launch("ls2d_keys")) return 1;
    if (g.n < 2) return 0;
    for (int p = 0; p < P; p++) {  // the sorts share the temporary storage: they run in stream order
        size_t temp_bytes = ws_bytes;
        hipError_t e = hipcub::DeviceMergeSort::SortKeys(ws, temp_bytes, keys_sorted + (long)p * g.n, (int)g.n, Ls2dKeyLess(), s);
        if (e != hipSuccess) {
            set_error("ls2d_sorted_keys: merge sort: %s", hipGetErrorString(e));
            return 1;
        }
    }
    return check_launch("ls2d_sort");
}

/* Host half (plain C++, no device access).  keys_host: P * n sorted keys (n = mvd_ls2d_num_cells), problem after problem.
 * bars [P][V + T][4] int32 (see ls2d_put): rows [0, V) are the dimension-0 bars in vertex order (the essential bar dies at
 * +inf / -inf, death vertex -1), rows [V, V + T) the dimension-1 bars in the order of the triangle that kills them.  Values
 * are in the sign of the input (the flip of a super-level filtration undone).  edge_row [P][E]: the bar row each edge is an
 * endpoint of (< V: the death of that dimension-0 bar; >= V: the birth of that dimension-1 bar). */
int mvd_ls2d_pair_host(const uint64_t *keys_host, int P, int H, int W, int sublevel, int maxdim, int32_t *bars,
                       int32_t *edge_row, int n_threads) {
    MVD_REQUIRE(keys_host && bars && P > 0 && H > 0 && W > 0 && maxdim >= 0 && maxdim <= 1, "ls2d_pair_host: bad arguments");
    const Ls2dGeom g = ls2d_geom(H, W, maxdim);
    MVD_REQUIRE(edge_row || g.E == 0, "ls2d_pair_host: edge_row is null");
    MVD_REQUIRE(g.V < (1L << 30) && g.E + g.T < (1L << 30), "ls2d_pair_host: too many cells");
    std::vector<int> rc((size_t)P, 0);
    host_pool(P, n_threads, [&](int p) {
        rc[p] = ls2d_pair_one(keys_host + (long)p * g.n, g, sublevel, bars + (long)p * (g.V + g.T) * 4,
                              edge_row + (long)p * g.E);
    });
    for (int p = 0; p < P; p++)
        MVD_REQUIRE(rc[p] == 0, "ls2d_pair_host: the keys of problem %d are not a sorted filtration of the %dx%d grid", p, W, H);
    return 0;
}

int mvd_ls2d_topk(const int32_t *bars, int P, int H, int W, int maxdim, int sublevel, int k, float *lengths, int32_t *index,
                  void *stream) {
    MVD_REQUIRE(bars && lengths && index && P > 0 && H > 0 && W > 0, "ls2d_topk: bad arguments");
    MVD_REQUIRE(reinterpret_cast<uintptr_t>(bars) % 16 == 0, "ls2d_topk: bars must be 16-byte aligned");
    MVD_REQUIRE(k >= 1 && k <= LS2D_MAX_K, "ls2d_topk: k must be in 1..%d (got %d)", LS2D_MAX_K, k);
    const Ls2dGeom g = ls2d_geom(H, W, maxdim);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_ls2d_topk, dim3(2 * P), dim3(1024), 0, s, bars, g.V, g.T, sublevel, k, lengths, index);
    return check_launch("ls2d_topk");
}

int mvd_ls2d_topk_bwd(const float *g_lengths, const int32_t *index, int P, int H, int W, int maxdim, int sublevel, int k,
                      float *g_bars, void *stream) {
    MVD_REQUIRE(g_lengths && index && g_bars && P > 0 && H > 0 && W > 0 && k >= 1 && k <= LS2D_MAX_K, "ls2d_topk_bwd: bad arguments");
    const Ls2dGeom g = ls2d_geom(H, W, maxdim);
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(g_bars, 0, sizeof(float) * 2 * (size_t)P * (size_t)(g.V + g.T), s) != hipSuccess) {
        set_error("ls2d_topk_bwd: memset failed");
        return 1;
    }
    const long total = (long)P * 2 * k;
    hipLaunchKernelGGL(k_ls2d_topk_bwd, dim3(cdiv(total, 256)), dim3(256), 0, s, g_lengths, index, g.V, g.T, sublevel, k, total,
                       g_bars);
    return check_launch("ls2d_topk_bwd");
}

int mvd_ls2d_topoloss_fwd(const float *lengths, const int32_t *label, int B, const int *idx, int n_idx, int n_label, int k,
                          float *out, void *stream) {
    Ls2dChannels ch;
    MVD_REQUIRE(lengths && label && out && B > 0 && k >= 1 && k <= LS2D_MAX_K, "ls2d_topoloss_fwd: bad arguments");
    if (ls2d_channels(idx, n_idx, n_label, &ch, "ls2d_topoloss_fwd")) return 2;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_ls2d_topoloss_fwd, dim3(1), dim3(256), 0, s, lengths, label, B, ch, n_label, k, out);
    return check_launch("ls2d_topoloss_fwd");
}

/* grad [B][C][H][W] is overwritten: zero except at the critical vertices of the selected bars of class idx + 1 */
int mvd_ls2d_topoloss_bwd(const float *lengths, const int32_t *index, const int32_t *bars, const int32_t *label,
                          const float *g_out, int B, int C, int H, int W, const int *idx, int n_idx, int n_label, int k,
                          int sublevel, float *grad, void *stream) {
    Ls2dChannels ch;
    MVD_REQUIRE(lengths && index && bars && label && g_out && grad && B > 0 && C > 0 && H > 0 && W > 0 && k >= 1 &&
                    k <= LS2D_MAX_K,
                "ls2d_topoloss_bwd: bad arguments");
    if (ls2d_channels(idx, n_idx, n_label, &ch, "ls2d_topoloss_bwd")) return 2;
    for (int i = 0; i < n_idx; i++) MVD_REQUIRE(idx[i] + 1 < C, "ls2d_topoloss_bwd: class %d + 1 outside the %d channels", idx[i], C);
    const Ls2dGeom g = ls2d_geom(H, W, 1);
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(grad, 0, sizeof(float) * (size_t)B * C * (size_t)g.V, s) != hipSuccess) {
        set_error("ls2d_topoloss_bwd: memset failed");
        return 1;
    }
    hipLaunchKernelGGL(k_ls2d_topoloss_bwd, dim3(B * n_idx), dim3(4 * LS2D_MAX_K), 0, s, lengths, index, bars, label, g_out, B, C,
                       ch, n_label, k, g.V, g.T, sublevel, grad);
    return check_launch("ls2d_topoloss_bwd");
}

/* grad [B][C][H][W] is overwritten: zero on the planes that are no problem.  g1 may be NULL (maxdim 0). */
int mvd_ls2d_diagram_bwd(const float *g0, const float *g1, const int32_t *bars, const int32_t *edge_row, int B, int C, int H,
                         int W, const int *channels, int n_channels, int maxdim, float *grad, void *stream) {
    Ls2dChannels chs;
    MVD_REQUIRE(g0 && bars && grad && B > 0 && C > 0 && H > 0 && W > 0 && maxdim >= 0 && maxdim <= 1,
                "ls2d_diagram_bwd: bad arguments");
    if (ls2d_channels(channels, n_channels, C, &chs, "ls2d_diagram_bwd")) return 2;
    const Ls2dGeom g = ls2d_geom(H, W, maxdim);
    MVD_REQUIRE(edge_row || g.E == 0, "ls2d_diagram_bwd: edge_row is null");
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(grad, 0, sizeof(float) * (size_t)B * C * (size_t)g.V, s) != hipSuccess) {
        set_error("ls2d_diagram_bwd: memset failed");
        return 1;
    }
    const long total = (long)B * n_channels * g.V;
    hipLaunchKernelGGL(k_ls2d_diagram_bwd, dim3(cdiv(total, 256)), dim3(256), 0, s, g0, maxdim >= 1 ? g1 : nullptr, bars, edge_row,
                       B, C, chs, g, grad);
    return check_launch("ls2d_diagram_bwd");
}

int mvd_ls2d_count_bars(const int32_t *bars, int P, int H, int W, int sublevel, int32_t *counts, void *stream) {
    MVD_REQUIRE(bars && counts && P > 0 && H > 0 && W > 0, "ls2d_count_bars: bad arguments");
    MVD_REQUIRE(reinterpret_cast<uintptr_t>(bars) % 16 == 0, "ls2d_count_bars: bars must be 16-byte aligned");
    const Ls2dGeom g = ls2d_geom(H, W, 1);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_ls2d_count, dim3(P), dim3(1024), 0, s, bars, g.V, g.T, sublevel, counts);
    return check_launch("ls2d_count_bars");
}

int mvd_ls2d_onehot(const float *label, float *planes, int B, int C, long V, void *stream) {
    MVD_REQUIRE(label && planes && B > 0 && C > 0 && V > 0, "ls2d_onehot: bad arguments");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_ls2d_onehot, dim3(ew_blocks((long)B * C * V, 8192)), dim3(256), 0, s, label, planes, B, C, V);
    return check_launch("ls2d_onehot");
}
}
