// Fused InstanceNorm3d(affine) + LeakyReLU on NDHWC fp32 activations  (SURVEY K3/K4).
// HBM-bound: fwd = read x (stats) + read x + write y; bwd = read x,dy (sums) + read x,dy + write dx.
// Statistics: per-thread fp64 accumulation -> fixed-order LDS reduce -> per-block partials -> fixed-order finalize; the
// geometry, the row walk, the pre-activation and these reductions are those of norm_common.h (shared with batchnorm.hip and
// resblock.hip).  The single-launch (small), tile-statistics and scale / shift kernels are this file's own.
#include "norm_common.h"

namespace mvd {

// ---- pass 1 (fwd): partial[n][b][c][2] = (sum x, sum x^2) in fp64
template <int VEC, bool XB>
__global__ void k_in_stats(const float *__restrict__ x, double *__restrict__ partial, int C, int CG, int R, long V,
                           long chunk) {
    extern __shared__ double sm[];  // [R][C][2]
    const NormThread<VEC> t(CG, V, chunk);
    if (t.r < R) {
        double s[VEC] = {}, ss[VEC] = {};
        norm_moments<VEC, XB>(x, t.base(V, C), t.v0 + t.r, t.v1, R, C, s, ss);
        norm_row_store<VEC>(sm, C, t.c0(), t.r, s, ss);
    }
    norm_block_reduce<2>(sm, partial, C, R, (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// scale / shift (optional): the fused form scale = gamma * rstd, shift = beta - mean * scale of the bf16 path (the expression
// of k_in_scale_shift / k_in_finalize_tiles on the float-rounded mean and rstd)
__global__ void k_in_finalize(const double *__restrict__ partial, float *__restrict__ mean, float *__restrict__ rstd,
                              int C, int nblk, long V, float eps, const float *__restrict__ gamma = nullptr,
                              const float *__restrict__ beta = nullptr, float *__restrict__ scale = nullptr,
                              float *__restrict__ shift = nullptr) {
    // one wave per (n, c): lanes stride over the block partials, fixed shuffle tree (deterministic)
    const int n = blockIdx.y, c = blockIdx.x;
    double s[2];
    norm_wave_sum<2>(partial, C, c, (size_t)n * nblk, nblk, s);
    if (threadIdx.x != 0) return;
    double m = s[0] / (double)V;
    double var = s[1] / (double)V - m * m;
    if (var < 0) var = 0;
    const float mf = (float)m, rf = (float)(1.0 / sqrt(var + (double)eps));
    mean[(size_t)n * C + c] = mf;
    rstd[(size_t)n * C + c] = rf;
    if (scale) {
        const float sc = gamma[c] * rf;
        scale[(size_t)n * C + c] = sc;
        shift[(size_t)n * C + c] = fmaf(-mf, sc, beta[c]);
    }
}

// conv-epilogue statistics: per-tile partials [n][tile][C][2] (fp32 sums of <= 128 values each) -> per-block fp64
// partials [n][b][C][2] in the layout k_in_finalize reads.  Thread = (channel, tile row): consecutive threads read
// consecutive (sum, sum of squares) pairs of one tile (coalesced); rows are combined through LDS in a fixed order.
__global__ void k_in_tiles_reduce(const float *__restrict__ tile, double *__restrict__ partial, int C, int CW, int R,
                                  long ntiles, long chunk) {
    extern __shared__ double sm[];  // [R][CW][2]
    const int n = blockIdx.y, b = blockIdx.x, nblk = gridDim.x;
    const int tc = threadIdx.x % CW, r = threadIdx.x / CW;
    const long t0 = (long)b * chunk;
    long t1 = t0 + chunk;
    if (t1 > ntiles) t1 = ntiles;
    for (int c0 = 0; c0 < C; c0 += CW) {
        const int c = c0 + tc;
        double a = 0, q = 0;
        if (r < R && c < C) {
            const float *tp = tile + ((size_t)n * ntiles * C + c) * 2;
            long tt = t0 + r;
            for (; tt + 3L * R < t1; tt += 4L * R) {  // four tiles in flight, added in tile order
                const float2 v0 = *reinterpret_cast<const float2 *>(tp + (size_t)tt * C * 2);
                const float2 v1 = *reinterpret_cast<const float2 *>(tp + (size_t)(tt + R) * C * 2);
                const float2 v2 = *reinterpret_cast<const float2 *>(tp + (size_t)(tt + 2L * R) * C * 2);
                const float2 v3 = *reinterpret_cast<const float2 *>(tp + (size_t)(tt + 3L * R) * C * 2);
                a += (double)v0.x; q += (double)v0.y;
                a += (double)v1.x; q += (double)v1.y;
                a += (double)v2.x; q += (double)v2.y;
                a += (double)v3.x; q += (double)v3.y;
            }
            for (; tt < t1; tt += R) {
                const float2 v = *reinterpret_cast<const float2 *>(tp + (size_t)tt * C * 2);
                a += (double)v.x;
                q += (double)v.y;
            }
        }
        __syncthreads();
        if (r < R) {
            sm[((size_t)r * CW + tc) * 2 + 0] = a;
            sm[((size_t)r * CW + tc) * 2 + 1] = q;
        }
        __syncthreads();
        if (r == 0 && c < C) {
            double sa = 0, sq = 0;
            for (int rr = 0; rr < R; rr++) {
                sa += sm[((size_t)rr * CW + tc) * 2 + 0];
                sq += sm[((size_t)rr * CW + tc) * 2 + 1];
            }
            const size_t o = (((size_t)n * nblk + b) * C + c) * 2;
            partial[o] = sa;
            partial[o + 1] = sq;
        }
    }
}

template <int VEC>
__global__ void k_in_apply(const float *__restrict__ x, const float *__restrict__ gamma,
                           const float *__restrict__ beta, const float *__restrict__ mean,
                           const float *__restrict__ rstd, float *__restrict__ y, int C, long V, float slope) {
    const int n = blockIdx.y;
    const long per_n = V * C / VEC;
    const float *xn = x + (size_t)n * V * C;
    float *yn = y + (size_t)n * V * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per_n; i += (long)gridDim.x * blockDim.x) {
        int c = (int)((i * VEC) % C);
        if (VEC == 4) {
            float4 q = reinterpret_cast<const float4 *>(xn)[i];
            float f[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float xh;
                const float z = norm_z(f[k], mean[(size_t)n * C + c + k], rstd[(size_t)n * C + c + k], gamma[c + k], beta[c + k], xh);
                f[k] = z > 0.f ? z : z * slope;
            }
            reinterpret_cast<float4 *>(yn)[i] = make_float4(f[0], f[1], f[2], f[3]);
        } else {
            float xh;
            const float z = norm_z(xn[i], mean[(size_t)n * C + c], rstd[(size_t)n * C + c], gamma[c], beta[c], xh);
            yn[i] = z > 0.f ? z : z * slope;
        }
    }
}

// row-mapped apply (C % 4 == 0): thread = (4-channel group g, row r); the per-channel parameters live in registers,
// each thread streams float4 rows v = v0 + r, v0 + r + R, ... of its block's voxel chunk (no per-element index math)
template <bool XB, bool YB>
__global__ void k_in_apply_rows(const float *__restrict__ x, const float *__restrict__ gamma,
                                const float *__restrict__ beta, const float *__restrict__ mean,
                                const float *__restrict__ rstd, float *__restrict__ y, int C, int CG, int R, long V,
                                long chunk, float slope) {
    const NormThread<4> t(CG, V, chunk);
    if (t.r >= R) return;
    const size_t base = t.base(V, C);
    float mu[4], rs[4], ga[4], be[4];
    norm_consts<4>(mu, rs, ga, be, mean, rstd, gamma, beta, (size_t)blockIdx.y * C, t.c0());
    long v = t.v0 + t.r;
    for (; v + 3L * R < t.v1; v += 4L * R) {  // four independent rows in flight
        float f[4][4];
#pragma unroll
        for (int u = 0; u < 4; u++) norm_ld<4, XB>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float xh;
                const float z = norm_z(f[u][i], mu[i], rs[i], ga[i], be[i], xh);
                f[u][i] = z > 0.f ? z : z * slope;
            }
            norm_st<4, YB>(y, base + (size_t)(v + (long)u * R) * C, f[u]);
        }
    }
    for (; v < t.v1; v += R) {
        float f[4];
        norm_ld<4, XB>(x, base + (size_t)v * C, f);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float xh;
            const float z = norm_z(f[i], mu[i], rs[i], ga[i], be[i], xh);
            f[i] = z > 0.f ? z : z * slope;
        }
        norm_st<4, YB>(y, base + (size_t)v * C, f);
    }
}

// ---- the backward of the LAST decoder block straight from the logit gradient (ops.NormActSegHeadFn, fp32): the fused seg
// head is the only consumer of the activated tensor a, so its gradient d a[v][c] = sum_k dl[n][k][v] * w[k][c] is formed in
// the two backward passes from the planar logit gradient (K floats per voxel) instead of being written and read back
// twice (C floats per voxel).  The expression and the k order are those of k_seghead_dx4 (loss.hip) on a zeroed
// accumulator, so d a is the value that kernel stores, bit for bit.
constexpr int HKMAX = 8;  // classes (KMAX of loss.hip); the class count is a template parameter here (registers)
template <int HK>
__device__ __forceinline__ void head_w_load(float4 (&wk)[HK], const float *__restrict__ w, int C, int g) {
#pragma unroll
    for (int k = 0; k < HK; k++) wk[k] = *reinterpret_cast<const float4 *>(w + (size_t)k * C + g * 4);
}
template <int HK>  // all class gradients of voxel v in flight at once
__device__ __forceinline__ void head_dl_load(float (&dq)[HK], const float *__restrict__ dl, int n, long V, long v) {
#pragma unroll
    for (int k = 0; k < HK; k++) dq[k] = dl[((size_t)n * HK + k) * V + v];
}
template <int HK>
__device__ __forceinline__ float4 head_da(const float (&dq)[HK], const float4 (&wk)[HK]) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < HK; k++) {
        a.x = fmaf(dq[k], wk[k].x, a.x);  // (explicit: k_seghead_dx4's a += d * w compiles to one fma per class, the first
        a.y = fmaf(dq[k], wk[k].y, a.y);  // on +0; left to contraction, some of these came out as a multiply and an add)
        a.z = fmaf(dq[k], wk[k].z, a.z);
        a.w = fmaf(dq[k], wk[k].w, a.w);
    }
    return a;
}
template <int HK>  // (into the float[4] of norm_ld)
__device__ __forceinline__ void head_da(float (&d)[4], const float (&dq)[HK], const float4 (&wk)[HK]) {
    const float4 a = head_da(dq, wk);
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
}

#ifndef MVD_IN_NRB
#define MVD_IN_NRB 4
#endif
constexpr int NRB = MVD_IN_NRB;  // rows in flight per thread in the backward apply pass
// HK > 0: dy is the planar logit gradient dl [N][HK][V] of the fused seg head and hw its weight [HK][C] (see head_da); the
// grid of in_bwd has at most 256 threads per block for C % 4 == 0
template <bool XB, bool YB, int HK = 0>
__global__ __launch_bounds__(HK > 0 ? 256 : 1024) void k_in_bwd_apply_rows(const float *__restrict__ x, const float *__restrict__ dy,
                                    const float *__restrict__ gamma, const float *__restrict__ beta,
                                    const float *__restrict__ mean, const float *__restrict__ rstd,
                                    const float *__restrict__ sums, float *__restrict__ dx, int C, int CG, int R, long V,
                                    long chunk, float slope, const float *__restrict__ hw = nullptr) {
    const int n = blockIdx.y;
    const NormThread<4> t(CG, V, chunk);
    if (t.r >= R) return;
    const size_t base = t.base(V, C);
    const float invV = 1.0f / (float)V;
    float mu[4], rs[4], ga[4], be[4], m1[4], m2[4];
    norm_consts<4>(mu, rs, ga, be, mean, rstd, gamma, beta, (size_t)n * C, t.c0());
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const size_t nc = (size_t)n * C + t.c0() + i;
        m1[i] = sums[nc * 2 + 0] * invV;
        m2[i] = sums[nc * 2 + 1] * invV;
    }
    float4 wk[HK > 0 ? HK : 1];
    if constexpr (HK > 0) head_w_load(wk, hw, C, t.g);
    long v = t.v0 + t.r;
    for (; v + (NRB - 1L) * R < t.v1; v += (long)NRB * R) {  // NRB rows (2 NRB loads) in flight
        float f[NRB][4], d[NRB][4];
        if constexpr (HK > 0) {
            float dq[NRB][HK];
#pragma unroll
            for (int u = 0; u < NRB; u++) {
                norm_ld<4, XB>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
                head_dl_load(dq[u], dy, n, V, v + (long)u * R);
            }
#pragma unroll
            for (int u = 0; u < NRB; u++) head_da(d[u], dq[u], wk);
        } else {
#pragma unroll
            for (int u = 0; u < NRB; u++) {
                norm_ld<4, XB>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
                norm_ld<4, YB>(dy, base + (size_t)(v + (long)u * R) * C, d[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < NRB; u++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float xh;
                const float z = norm_z(f[u][i], mu[i], rs[i], ga[i], be[i], xh);
                const float dz = z > 0.f ? d[u][i] : d[u][i] * slope;
                f[u][i] = ga[i] * rs[i] * (dz - m1[i] - xh * m2[i]);
            }
            norm_st<4, XB>(dx, base + (size_t)(v + (long)u * R) * C, f[u]);
        }
    }
    for (; v < t.v1; v += R) {
        float f[4], d[4];
        norm_ld<4, XB>(x, base + (size_t)v * C, f);
        if constexpr (HK > 0) {
            float dq[HK];
            head_dl_load(dq, dy, n, V, v);
            head_da(d, dq, wk);
        } else
            norm_ld<4, YB>(dy, base + (size_t)v * C, d);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float xh;
            const float z = norm_z(f[i], mu[i], rs[i], ga[i], be[i], xh);
            const float dz = z > 0.f ? d[i] : d[i] * slope;
            f[i] = ga[i] * rs[i] * (dz - m1[i] - xh * m2[i]);
        }
        norm_st<4, XB>(dx, base + (size_t)v * C, f);
    }
}

// ---- bwd pass 1: partial[n][b][c][2] = (sum dz, sum dz*xhat)
// HK > 0 (VEC == 4): dy is the planar logit gradient dl [N][HK][V] of the fused seg head and hw its weight [HK][C] (see head_da)
template <int VEC, bool XB, bool YB, int HK = 0>
__global__ __launch_bounds__(HK > 0 ? 256 : 1024) void k_in_bwd_stats(const float *__restrict__ x, const float *__restrict__ dy,
                               const float *__restrict__ gamma, const float *__restrict__ beta,
                               const float *__restrict__ mean, const float *__restrict__ rstd,
                               double *__restrict__ partial, int C, int CG, int R, long V, long chunk, float slope,
                               const float *__restrict__ hw = nullptr) {
    static_assert(HK == 0 || VEC == 4, "the head form works on 4-channel groups");
    extern __shared__ double sm[];  // [R][C][2]
    const int n = blockIdx.y;
    const NormThread<VEC> t(CG, V, chunk);
    if (t.r < R) {
        double s[VEC] = {}, ss[VEC] = {};
        const size_t base = t.base(V, C);
        float mu[VEC], rs[VEC], ga[VEC], be[VEC];
        norm_consts<VEC>(mu, rs, ga, be, mean, rstd, gamma, beta, (size_t)n * C, t.c0());
        float4 wk[HK > 0 ? HK : 1];
        if constexpr (HK > 0) head_w_load(wk, hw, C, t.g);
        long v = t.v0 + t.r;
        if (VEC == 4) {
            for (; v + R < t.v1; v += 2L * R) {  // two rows (four loads) in flight per thread, accumulated in row order
                float f[2][VEC], d[2][VEC];
                if constexpr (HK > 0) {
                    float dq[2][HK];
#pragma unroll
                    for (int u = 0; u < 2; u++) norm_ld<VEC, XB>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
#pragma unroll
                    for (int u = 0; u < 2; u++) head_dl_load(dq[u], dy, n, V, v + (long)u * R);
#pragma unroll
                    for (int u = 0; u < 2; u++) head_da(d[u], dq[u], wk);
                } else {
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        norm_ld<VEC, XB>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
                        norm_ld<VEC, YB>(dy, base + (size_t)(v + (long)u * R) * C, d[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; u++)
#pragma unroll
                    for (int i = 0; i < VEC; i++) {
                        float xh;
                        const float z = norm_z(f[u][i], mu[i], rs[i], ga[i], be[i], xh);
                        const float dz = z > 0.f ? d[u][i] : d[u][i] * slope;
                        s[i] += (double)dz;
                        ss[i] += (double)dz * (double)xh;
                    }
            }
        }
        for (; v < t.v1; v += R) {
            float f[VEC], d[VEC];
            norm_ld<VEC, XB>(x, base + (size_t)v * C, f);
            if constexpr (HK > 0) {
                float dq[HK];
                head_dl_load(dq, dy, n, V, v);
                head_da(d, dq, wk);
            } else
                norm_ld<VEC, YB>(dy, base + (size_t)v * C, d);
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                float xh;
                const float z = norm_z(f[i], mu[i], rs[i], ga[i], be[i], xh);
                const float dz = z > 0.f ? d[i] : d[i] * slope;
                s[i] += (double)dz;
                ss[i] += (double)dz * (double)xh;
            }
        }
        norm_row_store<VEC>(sm, C, t.c0(), t.r, s, ss);
    }
    norm_block_reduce<2>(sm, partial, C, R, (size_t)n * gridDim.x + blockIdx.x);
}

// sums[n][c][2] (float) = (sum dz, sum dz*xhat); dgamma/dbeta over n
__global__ void k_in_bwd_finalize(const double *__restrict__ partial, float *__restrict__ sums,
                                  float *__restrict__ dgamma, float *__restrict__ dbeta, int N, int C, int nblk) {
    // one wave per channel: lanes stride over the block partials of each sample, fixed shuffle tree
    const int c = blockIdx.x;
    double tg = 0, tb = 0;
    for (int n = 0; n < N; n++) {
        double s[2];
        norm_wave_sum<2>(partial, C, c, (size_t)n * nblk, nblk, s);
        if (threadIdx.x == 0) {
            sums[((size_t)n * C + c) * 2 + 0] = (float)s[0];
            sums[((size_t)n * C + c) * 2 + 1] = (float)s[1];
        }
        tb += s[0];
        tg += s[1];
    }
    if (threadIdx.x == 0) {
        dgamma[c] = (float)tg;
        dbeta[c] = (float)tb;
    }
}

// conv-epilogue statistics of the bf16 z-marching conv (k_fwd16z<.., FUSE & 1>): per-workgroup partials [n][tile][C][2]
// (fp32) -> mean, rstd and the fused form scale = gamma * rstd, shift = beta - mean * scale, ONE launch: a wave per
// (n, c), lanes stride over the tiles, fp64, fixed shuffle tree (deterministic).
__global__ void k_in_finalize_tiles(const float *__restrict__ tile, const float *__restrict__ gamma,
                                    const float *__restrict__ beta, float *__restrict__ mean, float *__restrict__ rstd,
                                    float *__restrict__ scale, float *__restrict__ shift, int C, long ntiles, long V,
                                    float eps) {
    const int n = blockIdx.y, c = blockIdx.x;
    double a = 0, q = 0;
    const float2 *tp = reinterpret_cast<const float2 *>(tile) + (size_t)n * ntiles * C + c;
    long t = threadIdx.x;
    for (; t + 192 < ntiles; t += 256) {  // four partials in flight per lane, added in tile order
        const float2 v0 = tp[(size_t)t * C], v1 = tp[(size_t)(t + 64) * C], v2 = tp[(size_t)(t + 128) * C],
                     v3 = tp[(size_t)(t + 192) * C];
        a += (double)v0.x; q += (double)v0.y;
        a += (double)v1.x; q += (double)v1.y;
        a += (double)v2.x; q += (double)v2.y;
        a += (double)v3.x; q += (double)v3.y;
    }
    for (; t < ntiles; t += 64) {
        const float2 v = tp[(size_t)t * C];
        a += (double)v.x;
        q += (double)v.y;
    }
    a = wave_sum(a);
    q = wave_sum(q);
    if (threadIdx.x != 0) return;
    const double m = a / (double)V;
    double var = q / (double)V - m * m;
    if (var < 0) var = 0;
    const float mf = (float)m, rs = (float)(1.0 / sqrt(var + (double)eps));
    const size_t nc = (size_t)n * C + c;
    mean[nc] = mf;
    rstd[nc] = rs;
    const float sc = gamma[c] * rs;
    scale[nc] = sc;
    shift[nc] = fmaf(-mf, sc, beta[c]);
}

// y = bf16(lrelu(fma(x, scale[n][c], shift[n][c]))): the apply pass in the form the fused conv prologue uses (k_fwd16z<.., FUSE &
// 2>), so that a tensor normalised here and one normalised in a consumer's loader agree bit for bit.  bf16 in, bf16 out.
__global__ void k_in_apply_ss16(const unsigned short *__restrict__ x, const float *__restrict__ scale,
                                const float *__restrict__ shift, unsigned short *__restrict__ y, int C, int CG, int R, long V,
                                long chunk, float slope) {
    const int n = blockIdx.y;
    const NormThread<4> t(CG, V, chunk);
    if (t.r >= R) return;
    const size_t base = t.base(V, C);
    float sc[4], sh[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        sc[i] = scale[(size_t)n * C + t.c0() + i];
        sh[i] = shift[(size_t)n * C + t.c0() + i];
    }
    long v = t.v0 + t.r;
    for (; v + 3L * R < t.v1; v += 4L * R) {  // four independent rows in flight
        float f[4][4];
#pragma unroll
        for (int u = 0; u < 4; u++) norm_ld<4, true>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float z = fmaf(f[u][i], sc[i], sh[i]);
                f[u][i] = fmaxf(z, z * slope);
            }
            norm_st<4, true>(y, base + (size_t)(v + (long)u * R) * C, f[u]);
        }
    }
    for (; v < t.v1; v += R) {
        float f[4];
        norm_ld<4, true>(x, base + (size_t)v * C, f);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float z = fmaf(f[i], sc[i], sh[i]);
            f[i] = fmaxf(z, z * slope);
        }
        norm_st<4, true>(y, base + (size_t)v * C, f);
    }
}

template <int VEC>
__global__ void k_in_bwd_apply(const float *__restrict__ x, const float *__restrict__ dy,
                               const float *__restrict__ gamma, const float *__restrict__ beta,
                               const float *__restrict__ mean, const float *__restrict__ rstd,
                               const float *__restrict__ sums, float *__restrict__ dx, int C, long V, float slope) {
    const int n = blockIdx.y;
    const long per_n = V * C / VEC;
    const size_t off = (size_t)n * V * C;
    const float invV = 1.0f / (float)V;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per_n; i += (long)gridDim.x * blockDim.x) {
        int c = (int)((i * VEC) % C);
        float f[VEC], d[VEC];
        if (VEC == 4) {
            float4 q = reinterpret_cast<const float4 *>(x + off)[i];
            float4 e = reinterpret_cast<const float4 *>(dy + off)[i];
            f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
            d[0] = e.x; d[1] = e.y; d[2] = e.z; d[3] = e.w;
        } else {
            f[0] = x[off + i];
            d[0] = dy[off + i];
        }
#pragma unroll
        for (int k = 0; k < VEC; k++) {
            size_t nc = (size_t)n * C + c + k;
            float rs = rstd[nc], xh;
            float z = norm_z(f[k], mean[nc], rs, gamma[c + k], beta[c + k], xh);
            float dz = z > 0.f ? d[k] : d[k] * slope;
            float m1 = sums[nc * 2 + 0] * invV, m2 = sums[nc * 2 + 1] * invV;
            f[k] = gamma[c + k] * rs * (dz - m1 - xh * m2);
        }
        if (VEC == 4)
            reinterpret_cast<float4 *>(dx + off)[i] = make_float4(f[0], f[1], f[2], f[3]);
        else
            dx[off + i] = f[0];
    }
}

// ---- small volumes (the 16^3 and deeper stages): ONE launch per direction instead of three.  A workgroup owns SMW float4
// lanes (16 channels, 64 contiguous bytes of every voxel row) of one sample; thread (lane gl, row r) keeps rows r, r + RP,
// ... (at most MAXR) in registers, so x (and dy) are read once.  Sums: per thread in fp64 in row order, a fixed xor
// tree over the 16 rows of a wave, then the waves in ascending order -- every thread ends with the same totals, no
// atomics.  mean / rstd with the arithmetic of k_in_finalize, y with that of k_in_apply_rows, dx with that of
// k_in_bwd_apply_rows on the float-rounded sums, dgamma / dbeta over n in ascending order as k_in_bwd_finalize.
constexpr int SMW = 4;
constexpr int SM_MAXR = 16;  // rows per thread: V <= 1024 on 256 threads (a 1024-thread form for V <= 4096 lost to the three
                             // launches at every size it added, profiles/r11_instnorm_small.txt)
__device__ __forceinline__ void small_reduce(double (&s)[4], double (&ss)[4], double (*sm)[SMW][8], int gl) {  // sm[4 waves]
#pragma unroll
    for (int off = SMW; off < 64; off <<= 1)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            s[i] += __shfl_xor(s[i], off);
            ss[i] += __shfl_xor(ss[i], off);
        }
    const int wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (nw == 1) return;
    if ((threadIdx.x & 63) < SMW)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            sm[wv][gl][2 * i] = s[i];
            sm[wv][gl][2 * i + 1] = ss[i];
        }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; i++) s[i] = ss[i] = 0.0;
    for (int w = 0; w < nw; w++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            s[i] += sm[w][gl][2 * i];
            ss[i] += sm[w][gl][2 * i + 1];
        }
}

template <int MAXR>
__global__ __launch_bounds__(256) void k_in_small_fwd(const float *__restrict__ x, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, float *__restrict__ y,
                                                       float *__restrict__ mean, float *__restrict__ rstd, int C, long V,
                                                       float eps, float slope) {
    __shared__ double sm[4][SMW][8];
    const int n = blockIdx.y, gl = threadIdx.x % SMW, r = threadIdx.x / SMW, RP = blockDim.x / SMW;
    const int g = blockIdx.x * SMW + gl;
    const bool act = g < (C >> 2);  // (the last workgroup of a C that is no multiple of 16)
    const size_t base = ((size_t)n * V) * C + (size_t)g * 4;
    float4 q[MAXR];
#pragma unroll
    for (int j = 0; j < MAXR; j++) {
        const long v = r + (long)j * RP;
        q[j] = (act && v < V) ? ld4<false>(x, base + (size_t)v * C) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    double s[4] = {0, 0, 0, 0}, ss[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < MAXR; j++) {  // (rows past V hold zeros: they add nothing)
        const float f[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            s[i] += (double)f[i];
            ss[i] += (double)f[i] * (double)f[i];
        }
    }
    small_reduce(s, ss, sm, gl);
    if (!act) return;
    float mu[4], rs[4], ga[4], be[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double m = s[i] / (double)V;
        double var = ss[i] / (double)V - m * m;
        if (var < 0) var = 0;
        mu[i] = (float)m;
        rs[i] = (float)(1.0 / sqrt(var + (double)eps));
        ga[i] = gamma[g * 4 + i];
        be[i] = beta[g * 4 + i];
    }
    if (r == 0)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            mean[(size_t)n * C + g * 4 + i] = mu[i];
            rstd[(size_t)n * C + g * 4 + i] = rs[i];
        }
#pragma unroll
    for (int j = 0; j < MAXR; j++) {
        const long v = r + (long)j * RP;
        if (v < V) {
            float f[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float xh;
                const float z = norm_z(f[i], mu[i], rs[i], ga[i], be[i], xh);
                f[i] = z > 0.f ? z : z * slope;
            }
            st4<false>(y, base + (size_t)v * C, f[0], f[1], f[2], f[3]);
        }
    }
}

template <int MAXR>
__global__ __launch_bounds__(256) void k_in_small_bwd(const float *__restrict__ x, const float *__restrict__ dy,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       const float *__restrict__ mean, const float *__restrict__ rstd,
                                                       float *__restrict__ dx, float *__restrict__ dgamma,
                                                       float *__restrict__ dbeta, int N, int C, long V, float slope) {
    __shared__ double sm[4][SMW][8];
    const int gl = threadIdx.x % SMW, r = threadIdx.x / SMW, RP = blockDim.x / SMW;
    const int g = blockIdx.x * SMW + gl;
    const bool act = g < (C >> 2);
    const int gc = act ? g : 0;  // (idle lanes read channel group 0's parameters and store nothing)
    const float invV = 1.0f / (float)V;
    float ga[4], be[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        ga[i] = gamma[gc * 4 + i];
        be[i] = beta[gc * 4 + i];
    }
    double tg[4] = {0, 0, 0, 0}, tb[4] = {0, 0, 0, 0};
    for (int n = 0; n < N; n++) {
        const size_t base = ((size_t)n * V) * C + (size_t)gc * 4;
        float mu[4], rs[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            mu[i] = mean[(size_t)n * C + gc * 4 + i];
            rs[i] = rstd[(size_t)n * C + gc * 4 + i];
        }
        float4 q[MAXR], e[MAXR];
#pragma unroll
        for (int j = 0; j < MAXR; j++) {
            const long v = r + (long)j * RP;
            const bool in = act && v < V;
            q[j] = in ? ld4<false>(x, base + (size_t)v * C) : make_float4(0.f, 0.f, 0.f, 0.f);
            e[j] = in ? ld4<false>(dy, base + (size_t)v * C) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        double s[4] = {0, 0, 0, 0}, ss[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < MAXR; j++) {  // q <- xhat, e <- dz (rows past V: dz = 0, they add nothing)
            float f[4] = {q[j].x, q[j].y, q[j].z, q[j].w}, d[4] = {e[j].x, e[j].y, e[j].z, e[j].w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float xh;
                const float z = norm_z(f[i], mu[i], rs[i], ga[i], be[i], xh);
                const float dz = z > 0.f ? d[i] : d[i] * slope;
                s[i] += (double)dz;
                ss[i] += (double)dz * (double)xh;
                f[i] = xh;
                d[i] = dz;
            }
            q[j] = make_float4(f[0], f[1], f[2], f[3]);
            e[j] = make_float4(d[0], d[1], d[2], d[3]);
        }
        if (n > 0) __syncthreads();  // the totals of sample n - 1 have been read
        small_reduce(s, ss, sm, gl);
        float m1[4], m2[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            m1[i] = (float)s[i] * invV;
            m2[i] = (float)ss[i] * invV;
            tb[i] += s[i];
            tg[i] += ss[i];
        }
#pragma unroll
        for (int j = 0; j < MAXR; j++) {
            const long v = r + (long)j * RP;
            if (act && v < V) {
                const float xh[4] = {q[j].x, q[j].y, q[j].z, q[j].w}, dz[4] = {e[j].x, e[j].y, e[j].z, e[j].w};
                float f[4];
#pragma unroll
                for (int i = 0; i < 4; i++) f[i] = ga[i] * rs[i] * (dz[i] - m1[i] - xh[i] * m2[i]);
                st4<false>(dx, base + (size_t)v * C, f[0], f[1], f[2], f[3]);
            }
        }
    }
    if (act && r == 0)
#pragma unroll
        for (int i = 0; i < 4; i++) {  // (scalar stores: the gradients may be slices of a flat buffer)
            dgamma[g * 4 + i] = (float)tg[i];
            dbeta[g * 4 + i] = (float)tb[i];
        }
}

}  // namespace mvd

using namespace mvd;

// ---- single-launch selection (MVD_IN_SMALL=0: always the three-launch form).  The default limit is where the single launch
// stopped winning on MI355X (tools/bench_instnorm_small.py, profiles/r11_instnorm_small.txt); MVD_IN_SMALL_MAX moves it.
constexpr long kInSmallMaxDefault = 327680;  // voxels x channels per sample (8x8x16 x 320 still won, 8x16x16 x 256 lost)
static long g_in_small_launches = 0;
static int in_small_threads(long V) {  // block size whose threads hold a sample's rows, 0: too many voxels
    for (int t = 64; t <= 256; t *= 4)
        if ((long)(t / SMW) * SM_MAXR >= V) return t;
    return 0;
}
static long g_in_small_max = -1;  // < 0: from the environment at first use
// nb: batch size of a BACKWARD launch, 0 for the forward.  The limit was measured at batch 2.  The forward grid has a
// workgroup per (16 channels, sample) and scales with the batch as the three launches do; the backward grid has C / 16
// workgroups that walk the samples one after the other (the order of dgamma / dbeta), so its time grows with N where the
// three launches spread over the chip: past two samples the backward limit shrinks with 2 / N (reasoned, not measured).
static int in_small_ok(long V, int C, int nb = 0) {
    static const int on = getenv("MVD_IN_SMALL") ? atoi(getenv("MVD_IN_SMALL")) : 1;
    if (g_in_small_max < 0)
        g_in_small_max = getenv("MVD_IN_SMALL_MAX") ? atol(getenv("MVD_IN_SMALL_MAX")) : kInSmallMaxDefault;
    if (!on || C % 4 != 0 || V <= 0) return 0;
    const long elems = V * C;
    if (nb > 2 ? elems * nb > 2 * g_in_small_max : elems > g_in_small_max) return 0;
    return in_small_threads(V);
}

// ---- the launch plan: which kernels an entry point runs and on which grids.  ALL of that arithmetic is here; the launch
// code below consumes an InPlan and mvd_instnorm_plan copies it out (tests/instnorm_ref.py restates it).
struct InPlan {
    int stats = MVD_IN_NONE, apply = MVD_IN_NONE;  // MVD_IN_* of the header
    int threads = 0, R = 0, CG = 0;                // block of the row-mapped kernels (norm_geom); the single launch: its own
    long nblk = 0, chunk = 0;                      // block partials per sample the finalize kernel sums; voxels per block
    long agrid = 0, achunk = 0;                    // apply pass: blocks per sample, voxels per block (0: grid stride)
    long tgrid = 0, tchunk = 0;                    // tile pass: blocks per sample, tiles per block
    int CW = 0, R2 = 0;                            // k_in_tiles_reduce: channels and tile rows of a 256-thread block
    int wblk = 0;                                  // norm_geom's nblk: the workspace holds N * wblk * C * 2 doubles
    size_t lds = 0;                                // LDS bytes of the statistics kernels
};

static void plan_apply_scalar(InPlan &p, int N, long V, int C) {  // C % 4 != 0: 256 threads, grid stride over the elements
    const long bx = cdiv(V * C, 256), cap = 4096 / N > 0 ? 4096 / N : 1;
    p.agrid = bx > cap ? cap : bx;
    p.achunk = 0;
}

static void plan_tiles_reduce(InPlan &p, long ntiles, int C) {
    long nb = (ntiles + 63) / 64;
    if (nb > p.wblk) nb = p.wblk;  // the workspace holds N * wblk * C * 2 doubles
    if (nb > 64) nb = 64;
    p.tchunk = (ntiles + nb - 1) / nb;
    p.tgrid = (ntiles + p.tchunk - 1) / p.tchunk;
    p.CW = C < 256 ? C : 256;
    p.R2 = 256 / p.CW;
    p.nblk = p.tgrid;
    p.chunk = 0;
}

// dir 0 forward, 1 backward (nb of in_small_ok: the batch); see mvd_instnorm_plan in the header for the entry point each
// combination of arguments stands for.  Refuses (status 2, message) what that entry point refuses by shape or type.
static int in_plan(InPlan &p, const char *who, int dir, int N, long V, int C, bool xb, bool yb, long ntiles, bool head) {
    MVD_REQUIRE(N > 0 && N <= 65535 && V > 0 && C > 0 && C <= 1024, "%s: bad shape N=%d V=%ld C=%d", who, N, V, C);
    MVD_REQUIRE(dir == 0 || dir == 1, "%s: direction %d", who, dir);
    MVD_REQUIRE(ntiles >= 0 && (dir == 0 || ntiles == 0), "%s: tile statistics (%ld tiles) belong to the forward", who, ntiles);
    const bool v4 = C % 4 == 0;
    MVD_REQUIRE(v4 || !(xb || yb), "%s: bf16 I/O needs C %% 4 == 0", who);
    MVD_REQUIRE(!xb || yb || (dir == 0 && head), "%s: a bf16 x goes with a bf16 y / dy", who);
    const NormGeom g = norm_geom(N, V, C);
    p = InPlan();
    p.threads = g.threads;
    p.R = g.R;
    p.CG = g.CG;
    p.nblk = p.wblk = g.nblk;
    p.chunk = g.chunk;
    p.lds = (size_t)g.R * C * 2 * sizeof(double);
    MVD_REQUIRE(p.lds <= 64 * 1024, "%s: C too large for the LDS reduce", who);
    if (dir == 0 && head) {  // statistics only: mvd_instnorm_stats_bf16 / mvd_instnorm_stats_from_tiles
        MVD_REQUIRE(ntiles > 0 ? !xb : v4, "%s: statistics alone need fp32 tiles or C %% 4 == 0", who);
        if (ntiles > 0) {
            p.stats = MVD_IN_TILES_REDUCE;
            plan_tiles_reduce(p, ntiles, C);
        } else
            p.stats = MVD_IN_STATS4;
        return 0;
    }
    MVD_REQUIRE(!head || (v4 && !xb && !yb), "%s: the logit-gradient form needs fp32, C %% 4 == 0 and K <= 8", who);
    if (!xb && !yb && !head) {
        if (const int th = in_small_ok(V, C, dir ? N : 0)) {  // (tile statistics, if any, are not needed)
            p.stats = p.apply = dir ? MVD_IN_SMALL_BWD : MVD_IN_SMALL_FWD;
            p.threads = th;
            p.R = th / SMW;
            p.CG = SMW;
            p.nblk = 1;
            p.chunk = V;
            p.agrid = cdiv(C / 4, SMW);  // workgroups of 16 channels: per sample forward, in all backward
            p.achunk = V;
            p.lds = 0;
            return 0;
        }
    }
    if (dir == 1) {
        MVD_REQUIRE(!head || g.threads <= 256, "%s: block size of the logit-gradient form", who);
        p.stats = head ? MVD_IN_BWD_STATS_HEAD : v4 ? MVD_IN_BWD_STATS4 : MVD_IN_BWD_STATS1;
        p.apply = head ? MVD_IN_BWD_APPLY_HEAD : v4 ? MVD_IN_BWD_APPLY_ROWS : MVD_IN_BWD_APPLY1;
    } else if (ntiles > 0 && yb) {  // mvd_instnorm_finalize_tiles, then mvd_instnorm_lrelu_apply_bf16
        MVD_REQUIRE(xb, "%s: tile statistics with a bf16 output need a bf16 input", who);
        p.stats = MVD_IN_FINALIZE_TILES;
        p.apply = MVD_IN_APPLY_SS16;
        p.nblk = p.chunk = 0;
        p.lds = 0;
        p.tgrid = 1;  // one wave per (n, c) takes all tiles
        p.tchunk = ntiles;
    } else {
        if (ntiles > 0) {
            p.stats = MVD_IN_TILES_REDUCE;
            plan_tiles_reduce(p, ntiles, C);
        } else
            p.stats = v4 ? MVD_IN_STATS4 : MVD_IN_STATS1;
        // bf16 in and out: the apply pass takes the scale / shift form -- ONE arithmetic for the stand-alone pass, the apply after
        // a conv's statistics epilogue and the loader prologues (conv, weight gradient, seg head), so fused and un-fused
        // networks agree bit for bit whichever kernel produced the statistics
        p.apply = !v4 ? MVD_IN_APPLY1 : xb ? MVD_IN_APPLY_SS16 : MVD_IN_APPLY_ROWS;
    }
    if (v4) {  // row-mapped apply passes: at most 8192 blocks over the batch
        p.achunk = norm_apply_chunk(g, 8192 / N);
        p.agrid = cdiv(V, p.achunk);
    } else
        plan_apply_scalar(p, N, V, C);
    return 0;
}

// the VEC == 4 kernels load float4 (fp32) or uint2 (bf16) at base + v * C: a stated requirement of x, y, dy and dx
static bool in_aligned(const void *ptr, bool bf16, int C) {
    return C % 4 != 0 || (reinterpret_cast<uintptr_t>(ptr) & (bf16 ? 7 : 15)) == 0;
}

extern "C" {

int mvd_instnorm_plan(int dir, int N, long V, int C, int x_is_bf16, int y_is_bf16, long ntiles, int head, long *plan) {
    MVD_REQUIRE(plan, "instnorm_plan: null pointer");
    InPlan p;
    if (const int rc = in_plan(p, "instnorm_plan", dir, N, V, C, x_is_bf16 != 0, y_is_bf16 != 0, ntiles, head != 0)) return rc;
    const long out[MVD_IN_PLAN_LEN] = {p.stats, p.apply,  p.threads, p.R,      p.CG, p.nblk, p.chunk,
                                       p.agrid, p.achunk, p.tgrid,   p.tchunk, p.CW, p.R2};
    for (int i = 0; i < MVD_IN_PLAN_LEN; i++) plan[i] = out[i];
    return 0;
}

int mvd_instnorm_single_launch(long V, int C) { return in_small_ok(V, C) > 0 ? 1 : 0; }
long mvd_instnorm_single_launches(void) { return g_in_small_launches; }
static long g_in_stats_pass_launches = 0;
long mvd_instnorm_stats_pass_launches(void) { return g_in_stats_pass_launches; }
int mvd_set_instnorm_small_max(long max_elems) {  // < 0: back to MVD_IN_SMALL_MAX / the default; 0: never
    g_in_small_max = max_elems < 0 ? -1 : max_elems;
    return 0;
}

int mvd_instnorm_nblk(int N, long V, int C) { return norm_geom(N, V, C).nblk; }

size_t mvd_instnorm_workspace_bytes(int N, long V, int C) {
    NormGeom g = norm_geom(N, V, C);
    // partials (doubles) + sums [N][C][2] floats
    return (size_t)N * g.nblk * C * 2 * sizeof(double) + (size_t)N * C * 2 * sizeof(float) + 256;
}

static int launch_tiles_reduce(const InPlan &p, const float *tile_stats, long ntiles, double *partial, float *mean, float *rstd,
                               int N, long V, int C, float eps, hipStream_t s) {
    hipLaunchKernelGGL(k_in_tiles_reduce, dim3((unsigned)p.tgrid, N), dim3(256), (size_t)p.R2 * p.CW * 2 * sizeof(double), s,
                       tile_stats, partial, C, p.CW, p.R2, ntiles, p.tchunk);
    if (check_launch("instnorm statistics from conv tiles")) return 1;
    hipLaunchKernelGGL(k_in_finalize, dim3(C, N), dim3(64), 0, s, partial, mean, rstd, C, (int)p.nblk, V, eps);
    return check_launch("instnorm finalize");
}

static int in_fwd(const float *x, bool xb, const float *gamma, const float *beta, float *y, bool yb, float *mean,
                  float *rstd, int N, long V, int C, float eps, float slope, void *ws, size_t ws_bytes, void *stream,
                  const float *tile_stats = nullptr, long ntiles = 0) {
    MVD_REQUIRE(x && gamma && beta && y && mean && rstd && ws, "instnorm_fwd: null pointer");
    InPlan p;
    if (const int rc = in_plan(p, "instnorm_fwd", 0, N, V, C, xb, yb, tile_stats ? ntiles : 0, false)) return rc;
    MVD_REQUIRE(ws_bytes >= mvd_instnorm_workspace_bytes(N, V, C), "instnorm_fwd: workspace too small");
    MVD_REQUIRE(in_aligned(x, xb, C) && in_aligned(y, yb, C),
                "instnorm_fwd: x and y must be 16-byte (fp32) / 8-byte (bf16) aligned for C %% 4 == 0");
    hipStream_t s = as_stream(stream);
    if (p.stats == MVD_IN_SMALL_FWD) {
        hipLaunchKernelGGL(k_in_small_fwd<SM_MAXR>, dim3(p.agrid, N), dim3(p.threads), 0, s, x, gamma, beta, y, mean, rstd, C, V,
                           eps, slope);
        g_in_small_launches++;
        return check_launch("instnorm forward (single launch)");
    }
    double *partial = reinterpret_cast<double *>(ws);
    const dim3 grid(p.nblk, N), agrid((unsigned)p.agrid, N);
    if (p.stats == MVD_IN_TILES_REDUCE) {
        // statistics came out of the producing conv's epilogue: no pass over x
        if (launch_tiles_reduce(p, tile_stats, ntiles, partial, mean, rstd, N, V, C, eps, s)) return 1;
    } else {
        if (p.stats == MVD_IN_STATS1)
            hipLaunchKernelGGL((k_in_stats<1, false>), grid, dim3(p.threads), p.lds, s, x, partial, C, p.CG, p.R, V, p.chunk);
        else if (xb)
            hipLaunchKernelGGL((k_in_stats<4, true>), grid, dim3(p.threads), p.lds, s, x, partial, C, p.CG, p.R, V, p.chunk);
        else
            hipLaunchKernelGGL((k_in_stats<4, false>), grid, dim3(p.threads), p.lds, s, x, partial, C, p.CG, p.R, V, p.chunk);
        g_in_stats_pass_launches++;
        if (check_launch("instnorm stats")) return 1;
        float *ss = reinterpret_cast<float *>(partial + (size_t)N * p.wblk * C * 2);
        const bool ssf = p.apply == MVD_IN_APPLY_SS16;
        hipLaunchKernelGGL(k_in_finalize, dim3(C, N), dim3(64), 0, s, partial, mean, rstd, C, (int)p.nblk, V, eps,
                           ssf ? gamma : nullptr, ssf ? beta : nullptr, ssf ? ss : nullptr, ssf ? ss + (size_t)N * C : nullptr);
        if (check_launch("instnorm finalize")) return 1;
        if (ssf) {
            hipLaunchKernelGGL(k_in_apply_ss16, agrid, dim3(p.threads), 0, s, reinterpret_cast<const unsigned short *>(x), ss,
                               ss + (size_t)N * C, reinterpret_cast<unsigned short *>(y), C, p.CG, p.R, V, p.achunk, slope);
            return check_launch("instnorm apply (scale / shift form)");
        }
    }
    if (p.apply == MVD_IN_APPLY_ROWS) {  // (a bf16 x takes k_in_apply_ss16 above: no bf16-input instantiation of this kernel)
        auto kern = yb ? k_in_apply_rows<false, true> : k_in_apply_rows<false, false>;
        hipLaunchKernelGGL(kern, agrid, dim3(p.threads), 0, s, x, gamma, beta, mean, rstd, y, C, p.CG, p.R, V, p.achunk, slope);
    } else
        hipLaunchKernelGGL(k_in_apply<1>, agrid, dim3(256), 0, s, x, gamma, beta, mean, rstd, y, C, V, slope);
    return check_launch("instnorm apply");
}

static int in_bwd(const float *x, bool xb, const float *dy, bool yb, const float *gamma, const float *beta,
                  const float *mean, const float *rstd, float *dx, float *dgamma, float *dbeta, int N, long V, int C,
                  float slope, void *ws, size_t ws_bytes, void *stream, const float *head_w = nullptr, int K = 0) {
    MVD_REQUIRE(x && dy && gamma && beta && mean && rstd && dx && dgamma && dbeta && ws, "instnorm_bwd: null pointer");
    InPlan p;
    if (const int rc = in_plan(p, "instnorm_bwd", 1, N, V, C, xb, yb, 0, head_w != nullptr)) return rc;
    MVD_REQUIRE(!head_w || (K > 0 && K <= HKMAX), "instnorm_bwd: the logit-gradient form needs fp32, C %% 4 == 0 and K <= 8");
    MVD_REQUIRE(ws_bytes >= mvd_instnorm_workspace_bytes(N, V, C), "instnorm_bwd: workspace too small");
    // (the logit gradient of the head form is planar and read one float at a time)
    MVD_REQUIRE(in_aligned(x, xb, C) && in_aligned(dx, xb, C) && (head_w || in_aligned(dy, yb, C)),
                "instnorm_bwd: x, dy and dx must be 16-byte (fp32) / 8-byte (bf16) aligned for C %% 4 == 0");
    hipStream_t s = as_stream(stream);
    if (p.stats == MVD_IN_SMALL_BWD) {
        hipLaunchKernelGGL(k_in_small_bwd<SM_MAXR>, dim3(p.agrid), dim3(p.threads), 0, s, x, dy, gamma, beta, mean, rstd, dx, dgamma,
                           dbeta, N, C, V, slope);
        g_in_small_launches++;
        return check_launch("instnorm backward (single launch)");
    }
    double *partial = reinterpret_cast<double *>(ws);
    float *sums = reinterpret_cast<float *>(partial + (size_t)N * p.wblk * C * 2);
    const dim3 grid(p.nblk, N), agrid((unsigned)p.agrid, N);
    if (p.stats == MVD_IN_BWD_STATS_HEAD) {
#define MVD_HEAD_STATS(KK)                                                                                                      \
    case KK:                                                                                                                    \
        hipLaunchKernelGGL((k_in_bwd_stats<4, false, false, KK>), grid, dim3(p.threads), p.lds, s, x, dy, gamma, beta, mean,    \
                           rstd, partial, C, p.CG, p.R, V, p.chunk, slope, head_w);                                             \
        break;
        switch (K) {
            MVD_HEAD_STATS(1) MVD_HEAD_STATS(2) MVD_HEAD_STATS(3) MVD_HEAD_STATS(4)
            MVD_HEAD_STATS(5) MVD_HEAD_STATS(6) MVD_HEAD_STATS(7) MVD_HEAD_STATS(8)
        }
#undef MVD_HEAD_STATS
    } else if (p.stats == MVD_IN_BWD_STATS4) {
        auto kern = xb ? k_in_bwd_stats<4, true, true> : (yb ? k_in_bwd_stats<4, false, true> : k_in_bwd_stats<4, false, false>);
        hipLaunchKernelGGL(kern, grid, dim3(p.threads), p.lds, s, x, dy, gamma, beta, mean, rstd, partial, C, p.CG, p.R, V,
                           p.chunk, slope, (const float *)nullptr);
    } else
        hipLaunchKernelGGL((k_in_bwd_stats<1, false, false>), grid, dim3(p.threads), p.lds, s, x, dy, gamma, beta, mean, rstd,
                           partial, C, p.CG, p.R, V, p.chunk, slope);
    if (check_launch("instnorm bwd stats")) return 1;
    hipLaunchKernelGGL(k_in_bwd_finalize, dim3(C), dim3(64), 0, s, partial, sums, dgamma, dbeta, N, C, (int)p.nblk);
    if (check_launch("instnorm bwd finalize")) return 1;
    if (p.apply == MVD_IN_BWD_APPLY_HEAD) {
#define MVD_HEAD_APPLY(KK)                                                                                                      \
    case KK:                                                                                                                    \
        hipLaunchKernelGGL((k_in_bwd_apply_rows<false, false, KK>), agrid, dim3(p.threads), 0, s, x, dy, gamma, beta, mean,     \
                           rstd, sums, dx, C, p.CG, p.R, V, p.achunk, slope, head_w);                                           \
        break;
        switch (K) {
            MVD_HEAD_APPLY(1) MVD_HEAD_APPLY(2) MVD_HEAD_APPLY(3) MVD_HEAD_APPLY(4)
            MVD_HEAD_APPLY(5) MVD_HEAD_APPLY(6) MVD_HEAD_APPLY(7) MVD_HEAD_APPLY(8)
        }
#undef MVD_HEAD_APPLY
    } else if (p.apply == MVD_IN_BWD_APPLY_ROWS) {  // (a bf16 x has a bf16 dy: no <true, false> instantiation)
        auto kern = xb ? k_in_bwd_apply_rows<true, true>
                       : (yb ? k_in_bwd_apply_rows<false, true> : k_in_bwd_apply_rows<false, false>);
        hipLaunchKernelGGL(kern, agrid, dim3(p.threads), 0, s, x, dy, gamma, beta, mean, rstd, sums, dx, C, p.CG, p.R, V,
                           p.achunk, slope, (const float *)nullptr);
    } else
        hipLaunchKernelGGL(k_in_bwd_apply<1>, agrid, dim3(256), 0, s, x, dy, gamma, beta, mean, rstd, sums, dx, C, V, slope);
    return check_launch("instnorm bwd apply");
}

int mvd_instnorm_lrelu_fwd(const float *x, const float *gamma, const float *beta, float *y, float *mean, float *rstd,
                           int N, long V, int C, float eps, float slope, void *ws, size_t ws_bytes, void *stream) {
    return in_fwd(x, false, gamma, beta, y, false, mean, rstd, N, V, C, eps, slope, ws, ws_bytes, stream);
}

int mvd_instnorm_lrelu_bwd(const float *x, const float *dy, const float *gamma, const float *beta, const float *mean,
                           const float *rstd, float *dx, float *dgamma, float *dbeta, int N, long V, int C,
                           float slope, void *ws, size_t ws_bytes, void *stream) {
    return in_bwd(x, false, dy, false, gamma, beta, mean, rstd, dx, dgamma, dbeta, N, V, C, slope, ws, ws_bytes, stream);
}

// InstanceNorm backward of the block whose only consumer is the fused seg head, from the head's logit gradient: dy of
// mvd_instnorm_lrelu_bwd is formed on the fly as dlogits^T w (what mvd_seghead_bwd_fused would store as dx); same grids,
// chunks and orders, so dx / dgamma / dbeta are bit-identical to the two-call form.  fp32, C % 4 == 0, K <= 8.
int mvd_instnorm_lrelu_bwd_head(const float *x, const float *dlogits, const float *w, int K, const float *gamma,
                                const float *beta, const float *mean, const float *rstd, float *dx, float *dgamma,
                                float *dbeta, int N, long V, int C, float slope, void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(w && (((uintptr_t)w) & 15) == 0, "instnorm_bwd_head: head weight (16-byte aligned) required");
    return in_bwd(x, false, dlogits, false, gamma, beta, mean, rstd, dx, dgamma, dbeta, N, V, C, slope, ws, ws_bytes, stream, w,
                  K);
}

int mvd_instnorm_lrelu_fwd_prestats(const float *x, const float *tile_stats, long ntiles, const float *gamma,
                                    const float *beta, float *y, float *mean, float *rstd, int N, long V, int C, float eps,
                                    float slope, void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(tile_stats && ntiles > 0, "instnorm_fwd_prestats: tile statistics required");
    return in_fwd(x, false, gamma, beta, y, false, mean, rstd, N, V, C, eps, slope, ws, ws_bytes, stream, tile_stats, ntiles);
}

int mvd_instnorm_finalize_tiles(const float *tile_stats, long ntiles, const float *gamma, const float *beta, float *mean,
                                float *rstd, float *scale, float *shift, int N, long V, int C, float eps, void *stream) {
    MVD_REQUIRE(tile_stats && gamma && beta && mean && rstd && scale && shift, "instnorm_finalize_tiles: null pointer");
    MVD_REQUIRE(ntiles > 0 && N > 0 && N <= 65535 && V > 0 && C > 0 && C <= 65535, "instnorm_finalize_tiles: bad shape");
    hipLaunchKernelGGL(k_in_finalize_tiles, dim3(C, N), dim3(64), 0, as_stream(stream), tile_stats, gamma, beta, mean, rstd,
                       scale, shift, C, ntiles, V, eps);
    return check_launch("instnorm finalize (conv tile statistics)");
}

// scale = gamma * rstd, shift = beta - mean * scale for [N][C] (the fused form of mean / rstd; same rounding as
// k_in_finalize_tiles)
__global__ void k_in_scale_shift(const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean,
                                 const float *__restrict__ rstd, float *__restrict__ scale, float *__restrict__ shift, int N,
                                 int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * C) return;
    const float sc = gamma[i % C] * rstd[i];
    scale[i] = sc;
    shift[i] = fmaf(-mean[i], sc, beta[i % C]);
}

int mvd_instnorm_stats_bf16(const void *x, int x_is_bf16, const float *gamma, const float *beta, float *mean, float *rstd,
                            float *scale, float *shift, int N, long V, int C, float eps, void *ws, size_t ws_bytes,
                            void *stream) {
    MVD_REQUIRE(x && gamma && beta && mean && rstd && scale && shift && ws, "instnorm_stats: null pointer");
    InPlan p;
    if (const int rc = in_plan(p, "instnorm_stats", 0, N, V, C, x_is_bf16 != 0, x_is_bf16 != 0, 0, true)) return rc;
    MVD_REQUIRE(ws_bytes >= mvd_instnorm_workspace_bytes(N, V, C), "instnorm_stats: workspace too small");
    MVD_REQUIRE(in_aligned(x, x_is_bf16 != 0, C), "instnorm_stats: x must be 16-byte (fp32) / 8-byte (bf16) aligned");
    hipStream_t s = as_stream(stream);
    double *partial = reinterpret_cast<double *>(ws);
    const float *xf = reinterpret_cast<const float *>(x);
    if (x_is_bf16)
        hipLaunchKernelGGL((k_in_stats<4, true>), dim3(p.nblk, N), dim3(p.threads), p.lds, s, xf, partial, C, p.CG, p.R, V, p.chunk);
    else
        hipLaunchKernelGGL((k_in_stats<4, false>), dim3(p.nblk, N), dim3(p.threads), p.lds, s, xf, partial, C, p.CG, p.R, V, p.chunk);
    if (check_launch("instnorm stats")) return 1;
    hipLaunchKernelGGL(k_in_finalize, dim3(C, N), dim3(64), 0, s, partial, mean, rstd, C, (int)p.nblk, V, eps, gamma, beta, scale,
                       shift);
    return check_launch("instnorm finalize");
}

// mean / rstd of an fp32 tensor from the fp32 conv's epilogue tiles (the statistics half of mvd_instnorm_lrelu_fwd_prestats:
// same launches, same order -- no apply pass; ops.NormActSegHeadFn in fp32)
int mvd_instnorm_stats_from_tiles(const float *tile_stats, long ntiles, float *mean, float *rstd, int N, long V, int C, float eps,
                                  void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(tile_stats && ntiles > 0 && mean && rstd && ws, "instnorm_stats_from_tiles: bad arguments");
    InPlan p;
    if (const int rc = in_plan(p, "instnorm_stats_from_tiles", 0, N, V, C, false, false, ntiles, true)) return rc;
    MVD_REQUIRE(ws_bytes >= mvd_instnorm_workspace_bytes(N, V, C), "instnorm_stats_from_tiles: workspace too small");
    return launch_tiles_reduce(p, tile_stats, ntiles, reinterpret_cast<double *>(ws), mean, rstd, N, V, C, eps, as_stream(stream));
}

int mvd_instnorm_lrelu_apply_bf16(const uint16_t *x, const float *scale, const float *shift, uint16_t *y, int N, long V,
                                  int C, float slope, void *stream) {
    MVD_REQUIRE(x && scale && shift && y, "instnorm_apply_bf16: null pointer");
    InPlan p;  // (the apply half of the bf16 tile form: its grid does not depend on the tile count)
    if (const int rc = in_plan(p, "instnorm_apply_bf16", 0, N, V, C, true, true, 1, false)) return rc;
    MVD_REQUIRE(in_aligned(x, true, C) && in_aligned(y, true, C), "instnorm_apply_bf16: x and y must be 8-byte aligned");
    hipLaunchKernelGGL(k_in_apply_ss16, dim3((unsigned)p.agrid, N), dim3(p.threads), 0, as_stream(stream), x, scale, shift, y, C,
                       p.CG, p.R, V, p.achunk, slope);
    return check_launch("instnorm apply (scale / shift form)");
}

int mvd_instnorm_lrelu_fwd_bf16(const void *x, int x_is_bf16, const float *gamma, const float *beta, uint16_t *y,
                                float *mean, float *rstd, int N, long V, int C, float eps, float slope, void *ws,
                                size_t ws_bytes, void *stream) {
    return in_fwd(reinterpret_cast<const float *>(x), x_is_bf16 != 0, gamma, beta, reinterpret_cast<float *>(y), true, mean,
                  rstd, N, V, C, eps, slope, ws, ws_bytes, stream);
}

int mvd_instnorm_lrelu_bwd_bf16(const void *x, int x_is_bf16, const uint16_t *dy, const float *gamma, const float *beta,
                                const float *mean, const float *rstd, void *dx, float *dgamma, float *dbeta, int N,
                                long V, int C, float slope, void *ws, size_t ws_bytes, void *stream) {
    return in_bwd(reinterpret_cast<const float *>(x), x_is_bf16 != 0, reinterpret_cast<const float *>(dy), true, gamma, beta,
                  mean, rstd, reinterpret_cast<float *>(dx), dgamma, dbeta, N, V, C, slope, ws, ws_bytes, stream);
}
}
