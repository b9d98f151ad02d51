// Fused BatchNorm3d(eps, affine, momentum, track_running_stats) + LeakyReLU on NDHWC activations (fp32 or bf16 storage).
// The normalisation of nnUNetTrainerBN.py:31-32 (norm_op = get_matching_batchnorm(conv_op) = nn.BatchNorm3d).
// HBM-bound like instnorm.hip: training fwd = read x (stats) + read x + write y; eval fwd = read x + write y;
// bwd = read x,dy (sums) + read x,dy + write dx.  Statistics are over the batch AND the volume (M = N * V values per
// channel): per-thread fp64 accumulation -> fixed-order LDS reduce -> per-block partials [n][b][c][2] -> ONE wave per
// channel sums all N * nblk partials in a fixed order.  No float atomics: run-to-run bit-identical.  The geometry, the
// row walk, the pre-activation and the reductions are those of norm_common.h, shared with instnorm.hip and resblock.hip;
// the kernels and the epilogues (running buffers, step counter, the EVAL root) are this file's own.
#include "norm_common.h"

namespace mvd {

static NormGeom bn_geom(int N, long V, int C) {
    NormGeom g = norm_geom(N, V, C);
    g.nblk = (int)cdiv(V, g.chunk);  // (no empty trailing block: one wave per channel sums ALL N * nblk partials)
    return g;
}

// ---- fwd pass 1: partial[n][b][c][2] = (sum x, sum x^2) in fp64
template <int VEC, bool XB>
__global__ __launch_bounds__(1024) void k_bn_stats(const void *__restrict__ x, double *__restrict__ partial, int C, int CG,
                                                   int R, long V, long chunk) {
    extern __shared__ double sm[];  // [R][C][2]
    const NormThread<VEC> t(CG, V, chunk);
    if (t.r < R) {
        double s[VEC] = {}, ss[VEC] = {};
        norm_moments<VEC, XB>(x, t.base(V, C), t.v0 + t.r, t.v1, R, C, s, ss);
        norm_row_store<VEC>(sm, C, t.c0(), t.r, s, ss);
    }
    norm_block_reduce<2>(sm, partial, C, R, (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// one wave per channel: mean, rstd (biased variance, formed in fp64, clamped at 0), the running buffers
// (torch.nn.functional.batch_norm: running_var takes the UNBIASED variance) and the step counter
__global__ void k_bn_finalize(const double *__restrict__ partial, float *__restrict__ mean, float *__restrict__ rstd,
                              float *__restrict__ running_mean, float *__restrict__ running_var,
                              long long *__restrict__ num_batches_tracked, int C, long total, long M, float eps,
                              double momentum) {
    const int c = blockIdx.x;
    double s[2];
    norm_wave_sum<2>(partial, C, c, 0, (int)total, s);  // (total = N * nblk <= max(2048, N))
    if (threadIdx.x != 0) return;
    const double m = s[0] / (double)M;
    double var = s[1] / (double)M - m * m;
    if (var < 0) var = 0;
    mean[c] = (float)m;
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    const double unbiased = var * ((double)M / (double)(M - 1));
    running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * m);
    running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
    if (c == 0) num_batches_tracked[0] += 1;  // on the device: a graph replay advances it
}

// ---- apply: y = lrelu(fma(xhat, gamma, beta)), xhat = (x - mean) * rstd.  EVAL: mean = running_mean and rstd =
// 1 / sqrt(running_var + eps), formed per channel in the prologue (fp64 root, rounded once) -- the training arithmetic on
// the running statistics, so no x * scale - mean * scale cancellation.
template <int VEC, bool XB, bool YB, bool EVAL>
__global__ __launch_bounds__(1024) void k_bn_apply(const void *__restrict__ x, const float *__restrict__ gamma,
                                                   const float *__restrict__ beta, const float *__restrict__ mean,
                                                   const float *__restrict__ rstd_or_var, void *__restrict__ y, int C, int CG,
                                                   int R, long V, long chunk, float eps, float slope) {
    const NormThread<VEC> t(CG, V, chunk);
    if (t.r >= R) return;
    const size_t base = t.base(V, C);
    float mu[VEC], rs[VEC], ga[VEC], be[VEC];
    norm_consts<VEC>(mu, rs, ga, be, mean, rstd_or_var, gamma, beta, 0, t.c0());
    if (EVAL)
#pragma unroll
        for (int i = 0; i < VEC; i++) rs[i] = (float)(1.0 / sqrt((double)rs[i] + (double)eps));
    long v = t.v0 + t.r;
    for (; v + 3L * R < t.v1; v += 4L * R) {  // four independent rows in flight
        float f[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; u++) norm_ld<VEC, XB>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                float xh;
                const float z = norm_z(f[u][i], mu[i], rs[i], ga[i], be[i], xh);
                f[u][i] = z > 0.f ? z : z * slope;
            }
            norm_st<VEC, YB>(y, base + (size_t)(v + (long)u * R) * C, f[u]);
        }
    }
    for (; v < t.v1; v += R) {
        float f[VEC];
        norm_ld<VEC, XB>(x, base + (size_t)v * C, f);
#pragma unroll
        for (int i = 0; i < VEC; i++) {
            float xh;
            const float z = norm_z(f[i], mu[i], rs[i], ga[i], be[i], xh);
            f[i] = z > 0.f ? z : z * slope;
        }
        norm_st<VEC, YB>(y, base + (size_t)v * C, f);
    }
}

// ---- bwd pass 1: partial[n][b][c][2] = (sum dz, sum dz * xhat); z is re-computed for the LeakyReLU mask
template <int VEC, bool XB, bool YB>
__global__ __launch_bounds__(1024) void k_bn_bwd_stats(const void *__restrict__ x, const void *__restrict__ dy,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       const float *__restrict__ mean, const float *__restrict__ rstd,
                                                       double *__restrict__ partial, int C, int CG, int R, long V,
                                                       long chunk, float slope) {
    extern __shared__ double sm[];  // [R][C][2]
    const NormThread<VEC> t(CG, V, chunk);
    if (t.r < R) {
        double s[VEC] = {}, ss[VEC] = {};
        const size_t base = t.base(V, C);
        float mu[VEC], rs[VEC], ga[VEC], be[VEC];
        norm_consts<VEC>(mu, rs, ga, be, mean, rstd, gamma, beta, 0, t.c0());
        long v = t.v0 + t.r;
        for (; v + R < t.v1; v += 2L * R) {  // two rows (four loads) in flight per thread, accumulated in row order
            float f[2][VEC], d[2][VEC];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                norm_ld<VEC, XB>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
                norm_ld<VEC, YB>(dy, base + (size_t)(v + (long)u * R) * C, d[u]);
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
        for (; v < t.v1; v += R) {
            float f[VEC], d[VEC];
            norm_ld<VEC, XB>(x, base + (size_t)v * C, f);
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
    norm_block_reduce<2>(sm, partial, C, R, (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// one wave per channel over all n: sums[c][2] (float) = (sum dz, sum dz * xhat) = (dbeta, dgamma)
__global__ void k_bn_bwd_finalize(const double *__restrict__ partial, float *__restrict__ sums, float *__restrict__ dgamma,
                                  float *__restrict__ dbeta, int C, long total) {
    const int c = blockIdx.x;
    double s[2];
    norm_wave_sum<2>(partial, C, c, 0, (int)total, s);
    if (threadIdx.x != 0) return;
    sums[(size_t)c * 2 + 0] = (float)s[0];
    sums[(size_t)c * 2 + 1] = (float)s[1];
    dgamma[c] = (float)s[1];  // (scalar stores: the gradients may be slices of a flat buffer)
    dbeta[c] = (float)s[0];
}

// ---- bwd pass 2: dx = gamma * rstd * (dz - sum dz / M - xhat * sum dz xhat / M), in x's dtype
template <int VEC, bool XB, bool YB>
__global__ __launch_bounds__(1024) void k_bn_bwd_apply(const void *__restrict__ x, const void *__restrict__ dy,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       const float *__restrict__ mean, const float *__restrict__ rstd,
                                                       const float *__restrict__ sums, void *__restrict__ dx, int C, int CG,
                                                       int R, long V, long chunk, float invM, float slope) {
    const NormThread<VEC> t(CG, V, chunk);
    if (t.r >= R) return;
    const size_t base = t.base(V, C);
    float mu[VEC], rs[VEC], ga[VEC], be[VEC], m1[VEC], m2[VEC];
    norm_consts<VEC>(mu, rs, ga, be, mean, rstd, gamma, beta, 0, t.c0());
#pragma unroll
    for (int i = 0; i < VEC; i++) {
        m1[i] = sums[(size_t)(t.c0() + i) * 2 + 0] * invM;
        m2[i] = sums[(size_t)(t.c0() + i) * 2 + 1] * invM;
    }
    long v = t.v0 + t.r;
    for (; v + 3L * R < t.v1; v += 4L * R) {  // four rows (eight loads) in flight
        float f[4][VEC], d[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            norm_ld<VEC, XB>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
            norm_ld<VEC, YB>(dy, base + (size_t)(v + (long)u * R) * C, d[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                float xh;
                const float z = norm_z(f[u][i], mu[i], rs[i], ga[i], be[i], xh);
                const float dz = z > 0.f ? d[u][i] : d[u][i] * slope;
                f[u][i] = ga[i] * rs[i] * (dz - m1[i] - xh * m2[i]);
            }
            norm_st<VEC, XB>(dx, base + (size_t)(v + (long)u * R) * C, f[u]);
        }
    }
    for (; v < t.v1; v += R) {
        float f[VEC], d[VEC];
        norm_ld<VEC, XB>(x, base + (size_t)v * C, f);
        norm_ld<VEC, YB>(dy, base + (size_t)v * C, d);
#pragma unroll
        for (int i = 0; i < VEC; i++) {
            float xh;
            const float z = norm_z(f[i], mu[i], rs[i], ga[i], be[i], xh);
            const float dz = z > 0.f ? d[i] : d[i] * slope;
            f[i] = ga[i] * rs[i] * (dz - m1[i] - xh * m2[i]);
        }
        norm_st<VEC, XB>(dx, base + (size_t)v * C, f);
    }
}

static int bn_shape_ok(int N, long V, int C) { return N > 0 && N <= 65535 && V > 0 && C > 0 && C <= 1024; }

// kernel of the (VEC, x storage, y storage) combination
#define MVD_BN_PICK(KERN, v4, xb, yb, ...)                                                        \
    ((v4) ? ((xb) ? ((yb) ? KERN<4, true, true __VA_ARGS__> : KERN<4, true, false __VA_ARGS__>)   \
                  : ((yb) ? KERN<4, false, true __VA_ARGS__> : KERN<4, false, false __VA_ARGS__>)) \
          : ((xb) ? ((yb) ? KERN<1, true, true __VA_ARGS__> : KERN<1, true, false __VA_ARGS__>)   \
                  : ((yb) ? KERN<1, false, true __VA_ARGS__> : KERN<1, false, false __VA_ARGS__>)))

}  // namespace mvd

using namespace mvd;

extern "C" {

int mvd_batchnorm_nblk(int N, long V, int C) { return bn_shape_ok(N, V, C) ? bn_geom(N, V, C).nblk : 0; }

size_t mvd_batchnorm_workspace_bytes(int N, long V, int C) {
    if (!bn_shape_ok(N, V, C)) return 0;
    const NormGeom g = bn_geom(N, V, C);
    // partials [N][nblk][C][2] doubles + sums [C][2] floats
    return (size_t)N * g.nblk * C * 2 * sizeof(double) + (size_t)C * 2 * sizeof(float) + 256;
}

int mvd_batchnorm_lrelu_fwd(const void *x, int x_is_bf16, const float *gamma, const float *beta, void *y, int y_is_bf16,
                            float *mean, float *rstd, float *running_mean, float *running_var,
                            int64_t *num_batches_tracked, int N, long V, int C, float eps, double momentum, float slope,
                            void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(x && gamma && beta && y && mean && rstd && running_mean && running_var && num_batches_tracked && ws,
                "batchnorm_fwd: null pointer (affine parameters and running buffers are required)");
    MVD_REQUIRE(bn_shape_ok(N, V, C), "batchnorm_fwd: bad shape N=%d V=%ld C=%d", N, V, C);
    MVD_REQUIRE((long)N * V > 1, "batchnorm_fwd: expected more than 1 value per channel when training (N * V == 1)");
    MVD_REQUIRE(momentum >= 0.0 && momentum <= 1.0, "batchnorm_fwd: momentum %g outside [0, 1]", momentum);
    MVD_REQUIRE(ws_bytes >= mvd_batchnorm_workspace_bytes(N, V, C), "batchnorm_fwd: workspace too small");
    const NormGeom g = bn_geom(N, V, C);
    const bool v4 = g.vec == 4, xb = x_is_bf16 != 0, yb = y_is_bf16 != 0;
    hipStream_t s = as_stream(stream);
    double *partial = reinterpret_cast<double *>(ws);
    const size_t sm = (size_t)g.R * C * 2 * sizeof(double);  // <= 16 KiB for C <= 1024
    auto stats = v4 ? (xb ? k_bn_stats<4, true> : k_bn_stats<4, false>) : (xb ? k_bn_stats<1, true> : k_bn_stats<1, false>);
    hipLaunchKernelGGL(stats, dim3(g.nblk, N), dim3(g.threads), sm, s, x, partial, C, g.CG, g.R, V, g.chunk);
    if (check_launch("batchnorm stats")) return 1;
    hipLaunchKernelGGL(k_bn_finalize, dim3(C), dim3(64), 0, s, partial, mean, rstd, running_mean, running_var,
                       reinterpret_cast<long long *>(num_batches_tracked), C, (long)N * g.nblk, (long)N * V, eps, momentum);
    if (check_launch("batchnorm finalize")) return 1;
    const long chunk2 = norm_apply_chunk(g, 8192 / N);
    auto apply = MVD_BN_PICK(k_bn_apply, v4, xb, yb, , false);
    hipLaunchKernelGGL(apply, dim3((unsigned)cdiv(V, chunk2), N), dim3(g.threads), 0, s, x, gamma, beta, mean, rstd, y, C, g.CG,
                       g.R, V, chunk2, eps, slope);
    return check_launch("batchnorm apply");
}

int mvd_batchnorm_lrelu_eval(const void *x, int x_is_bf16, const float *gamma, const float *beta, void *y, int y_is_bf16,
                             const float *running_mean, const float *running_var, int N, long V, int C, float eps,
                             float slope, void *stream) {
    MVD_REQUIRE(x && gamma && beta && y && running_mean && running_var,
                "batchnorm_eval: null pointer (affine parameters and running buffers are required)");
    MVD_REQUIRE(bn_shape_ok(N, V, C), "batchnorm_eval: bad shape N=%d V=%ld C=%d", N, V, C);
    const NormGeom g = bn_geom(N, V, C);
    const bool v4 = g.vec == 4, xb = x_is_bf16 != 0, yb = y_is_bf16 != 0;
    const long chunk2 = norm_apply_chunk(g, 8192 / N);
    auto apply = MVD_BN_PICK(k_bn_apply, v4, xb, yb, , true);
    hipLaunchKernelGGL(apply, dim3((unsigned)cdiv(V, chunk2), N), dim3(g.threads), 0, as_stream(stream), x, gamma, beta,
                       running_mean, running_var, y, C, g.CG, g.R, V, chunk2, eps, slope);
    return check_launch("batchnorm apply (running statistics)");
}

int mvd_batchnorm_lrelu_bwd(const void *x, int x_is_bf16, const void *dy, int y_is_bf16, const float *gamma,
                            const float *beta, const float *mean, const float *rstd, void *dx, float *dgamma, float *dbeta,
                            int N, long V, int C, float slope, void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(x && dy && gamma && beta && mean && rstd && dx && dgamma && dbeta && ws, "batchnorm_bwd: null pointer");
    MVD_REQUIRE(bn_shape_ok(N, V, C), "batchnorm_bwd: bad shape N=%d V=%ld C=%d", N, V, C);
    MVD_REQUIRE((long)N * V > 1, "batchnorm_bwd: expected more than 1 value per channel (N * V == 1)");
    MVD_REQUIRE(ws_bytes >= mvd_batchnorm_workspace_bytes(N, V, C), "batchnorm_bwd: workspace too small");
    const NormGeom g = bn_geom(N, V, C);
    const bool v4 = g.vec == 4, xb = x_is_bf16 != 0, yb = y_is_bf16 != 0;
    hipStream_t s = as_stream(stream);
    double *partial = reinterpret_cast<double *>(ws);
    float *sums = reinterpret_cast<float *>(partial + (size_t)N * g.nblk * C * 2);
    const size_t sm = (size_t)g.R * C * 2 * sizeof(double);
    auto stats = MVD_BN_PICK(k_bn_bwd_stats, v4, xb, yb);
    hipLaunchKernelGGL(stats, dim3(g.nblk, N), dim3(g.threads), sm, s, x, dy, gamma, beta, mean, rstd, partial, C, g.CG, g.R, V,
                       g.chunk, slope);
    if (check_launch("batchnorm bwd stats")) return 1;
    hipLaunchKernelGGL(k_bn_bwd_finalize, dim3(C), dim3(64), 0, s, partial, sums, dgamma, dbeta, C, (long)N * g.nblk);
    if (check_launch("batchnorm bwd finalize")) return 1;
    const long chunk2 = norm_apply_chunk(g, 8192 / N);
    auto apply = MVD_BN_PICK(k_bn_bwd_apply, v4, xb, yb);
    hipLaunchKernelGGL(apply, dim3((unsigned)cdiv(V, chunk2), N), dim3(g.threads), 0, s, x, dy, gamma, beta, mean, rstd, sums, dx,
                       C, g.CG, g.R, V, chunk2, (float)(1.0 / (double)((long)N * V)), slope);
    return check_launch("batchnorm bwd apply");
}
}
