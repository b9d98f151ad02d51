// What instnorm.hip, batchnorm.hip and resblock.hip share: the geometry of their row-mapped kernels, the row walk of a
// thread, THE pre-activation, and the fixed-order fp64 reductions.  Activations are [N,V,C] channel-last; a thread is
// (channel group g of VEC channels, row r), a block owns `chunk` voxels of one sample and its thread walks the rows
// v0 + r, v0 + r + R, ...  Statistics: per thread in fp64 in ascending row order (norm_moments) -> rows combined through
// LDS in ascending order (norm_block_reduce) -> block partials summed by one wave, lanes striding, fixed shuffle tree
// (norm_wave_sum).  No atomics: every sum has one association, so a graph replay repeats the eager step bit for bit.
#pragma once
#include "common.h"

namespace mvd {

struct NormGeom {
    int C, vec, CG, R, threads, nblk;
    long V, chunk;
};

static inline NormGeom norm_geom(int N, long V, int C) {
    NormGeom g;
    g.C = C;
    g.V = V;
    g.vec = (C % 4 == 0) ? 4 : 1;
    g.CG = C / g.vec;  // <= 256 (vec 4) or <= 1024 (scalar): every entry point requires C <= 1024
    g.R = 256 / g.CG;
    if (g.R < 1) g.R = 1;
    g.threads = ((g.R * g.CG + 63) / 64) * 64;  // <= 1024
    long want = 2048 / (N > 0 ? N : 1);
    if (want < 1) want = 1;
    long nblk = V / ((long)g.R * 16);  // statistics: at least 16 rows per thread
    if (nblk < 1) nblk = 1;
    if (nblk > want) nblk = want;
    g.nblk = (int)nblk;
    g.chunk = cdiv(V, nblk);
    return g;
}

// voxels per block of a streaming pass: about 8 rows per thread -- more, smaller chunks than the reducing passes (no
// reduction to amortise) -- on at most `cap` blocks per sample (the caller's: they differ, and they set grid sizes)
static inline long norm_apply_chunk(const NormGeom &g, long cap) {
    long nb = g.V / ((long)g.R * 8);
    if (nb > cap) nb = cap;
    if (nb < 1) nb = 1;
    return cdiv(g.V, nb);
}

// the thread of a row-mapped kernel on grid (blocks of `chunk` voxels, N): channels c0 .. c0 + VEC - 1 of the rows v0 + r,
// v0 + r + R, ... < v1 (rows r >= R of a block padded to whole waves have none); row v is at base(V, C) + v * C (formed
// by the caller behind its r < R guard: formed ahead of it, it is held in registers across the guard)
template <int VEC>
struct NormThread {
    int g, r;
    long v0, v1;
    __device__ __forceinline__ NormThread(int CG, long V, long chunk) {
        g = threadIdx.x % CG;
        r = threadIdx.x / CG;
        v0 = (long)blockIdx.x * chunk;
        v1 = v0 + chunk;
        if (v1 > V) v1 = V;
    }
    __device__ __forceinline__ int c0() const { return g * VEC; }
    __device__ __forceinline__ size_t base(long V, int C) const { return ((size_t)blockIdx.y * V) * C + (size_t)g * VEC; }
};

// VEC consecutive channels at element e of a float (BF = false) or bf16 (BF = true) tensor, as fp32
template <int VEC, bool BF>
__device__ __forceinline__ void norm_ld(const void *p, size_t e, float (&f)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 q = ld4<BF>(p, e);
        f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
    } else
        f[0] = ld1<BF>(p, e);
}
template <int VEC, bool BF>
__device__ __forceinline__ void norm_st(void *p, size_t e, const float (&f)[VEC]) {
    if constexpr (VEC == 4)
        st4<BF>(p, e, f[0], f[1], f[2], f[3]);
    else
        st1<BF>(p, e, f[0]);
}

// THE pre-activation z = xhat * gamma + beta; xh returns xhat = (x - mean) * rstd.  Explicit fmaf: the same rounding in
// every kernel that re-computes z, forward and backward, whatever the compiler contracts elsewhere.
__device__ __forceinline__ float norm_z(float x, float mu, float rs, float ga, float be, float &xh) {
    xh = (x - mu) * rs;
    return fmaf(xh, ga, be);
}

// the per-channel constants of a thread's channels c0 .. c0 + VEC - 1; row: offset of the sample's statistics (n * C
// where they are per sample, 0 where they are per channel)
template <int VEC>
__device__ __forceinline__ void norm_consts(float (&mu)[VEC], float (&rs)[VEC], float (&ga)[VEC], float (&be)[VEC],
                                            const float *__restrict__ mean, const float *__restrict__ rstd,
                                            const float *__restrict__ gamma, const float *__restrict__ beta, size_t row,
                                            int c0) {
#pragma unroll
    for (int i = 0; i < VEC; i++) {
        mu[i] = mean[row + c0 + i];
        rs[i] = rstd[row + c0 + i];
        ga[i] = gamma[c0 + i];
        be[i] = beta[c0 + i];
    }
}

// s += sum x, ss += sum x^2 over the rows v, v + R, ... < v1 of a thread, in fp64 in ascending row order: four rows
// in flight, then one at a time
template <int VEC, bool BF>
__device__ __forceinline__ void norm_moments(const void *__restrict__ x, size_t base, long v, long v1, int R, int C,
                                             double (&s)[VEC], double (&ss)[VEC]) {
    for (; v + 3L * R < v1; v += 4L * R) {
        float f[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; u++) norm_ld<VEC, BF>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                s[i] += (double)f[u][i];
                ss[i] += (double)f[u][i] * (double)f[u][i];
            }
    }
    for (; v < v1; v += R) {
        float f[VEC];
        norm_ld<VEC, BF>(x, base + (size_t)v * C, f);
#pragma unroll
        for (int i = 0; i < VEC; i++) {
            s[i] += (double)f[i];
            ss[i] += (double)f[i] * (double)f[i];
        }
    }
}

// The block combine, in two calls.  First the NS sums of a thread's rows (one double[VEC] per sum) -> its row of sm
// ([R][C][NS] doubles): by the threads r < R, BEHIND their guard -- sums that cross the guard are held in registers
// twice -- and from one array per sum: accumulated in one [NS][VEC] array, the backward kernels took up to 8 more
// registers (profiles/r25_norm_common.txt).
template <int VEC, typename... S>
__device__ __forceinline__ void norm_row_store(double *sm, int C, int c0, int r, const S &...s) {
    constexpr int NS = sizeof...(S);
    const double *p[NS] = {s...};
#pragma unroll
    for (int i = 0; i < VEC; i++)
#pragma unroll
        for (int k = 0; k < NS; k++) sm[((size_t)r * C + c0 + i) * NS + k] = p[k][i];
}
// ... then, by all threads of the block: partial[slot][c][NS] = the rows of sm added in ascending order
template <int NS>
__device__ __forceinline__ void norm_block_reduce(const double *sm, double *__restrict__ partial, int C, int R, size_t slot) {
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double q[NS];
#pragma unroll
        for (int k = 0; k < NS; k++) q[k] = 0;
        for (int rr = 0; rr < R; rr++)
#pragma unroll
            for (int k = 0; k < NS; k++) q[k] += sm[((size_t)rr * C + c) * NS + k];
#pragma unroll
        for (int k = 0; k < NS; k++) partial[(slot * C + c) * NS + k] = q[k];
    }
}

// out[k] = sum over the `count` block partials partial[first + j][c][k], by one wave: lane l takes j = l, l + 64, ... in
// ascending order, two partials in flight in two accumulators (j = l, l + 128, ... and j = l + 64, l + 192, ...; a last odd
// one joins the first), then the fixed shuffle tree over their sum.  Valid in lane 0.
template <int NS>
__device__ __forceinline__ void norm_wave_sum(const double *__restrict__ partial, int C, int c, size_t first, int count,
                                              double (&out)[NS]) {
    double a0[NS], a1[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) a0[k] = a1[k] = 0;
    int j = threadIdx.x;
    for (; j + 64 < count; j += 128) {
        const size_t o = ((first + j) * C + c) * NS, o1 = ((first + j + 64) * C + c) * NS;
        double v[NS], w[NS];
#pragma unroll
        for (int k = 0; k < NS; k++) {
            v[k] = partial[o + k];
            w[k] = partial[o1 + k];
        }
#pragma unroll
        for (int k = 0; k < NS; k++) {
            a0[k] += v[k];
            a1[k] += w[k];
        }
    }
    for (; j < count; j += 64) {
        const size_t o = ((first + j) * C + c) * NS;
#pragma unroll
        for (int k = 0; k < NS; k++) a0[k] += partial[o + k];
    }
#pragma unroll
    for (int k = 0; k < NS; k++) out[k] = wave_sum(a0[k] + a1[k]);
}

}  // namespace mvd
