// Fused BatchNorm3d(eps, affine, momentum, track_running_stats) + LeakyReLU on NDHWC activations (fp32 or bf16 storage).
// The normalisation of nnUNetTrainerBN.py:31-32 (norm_op = get_matching_batchnorm(conv_op) = nn.BatchNorm3d).
// HBM-bound like instnorm.hip: training fwd = read x (stats) + read x + write y; eval fwd = read x + write y;
// bwd = read x,dy (sums) + read x,dy + write dx.  Statistics are over the batch AND the volume (M = N * V values per
// channel): per-thread fp64 accumulation -> fixed-order LDS reduce -> per-block partials [n][b][c][2] -> ONE wave per
// channel sums all N * nblk partials in a fixed order.  No float atomics: run-to-run bit-identical.  Self-contained: shares
// only common.h with instnorm.hip.
#include "common.h"

namespace mvd {

struct BnGeom {
    int C, VEC, CG, R, threads, nblk;
    long V, chunk;
};

// thread = (channel group g of VEC channels, row r); a block owns `chunk` voxels of one sample
static BnGeom bn_geom(int N, long V, int C) {
    BnGeom g;
    g.C = C;
    g.V = V;
    g.VEC = (C % 4 == 0) ? 4 : 1;
    g.CG = C / g.VEC;  // C <= 1024: at most 256 groups of four, or up to 1023 scalar columns
    g.R = 256 / g.CG;
    if (g.R < 1) g.R = 1;
    g.threads = ((g.R * g.CG + 63) / 64) * 64;
    long want = 2048 / (N > 0 ? N : 1);
    if (want < 1) want = 1;
    long rows_min = (long)g.R * 16;  // at least 16 voxels per thread
    long nblk = V / rows_min;
    if (nblk < 1) nblk = 1;
    if (nblk > want) nblk = want;
    g.chunk = cdiv(V, nblk);
    g.nblk = (int)cdiv(V, g.chunk);  // (no empty trailing block)
    return g;
}

// the streaming passes take more, smaller chunks than the reducing ones (no reduction to amortise)
static long bn_apply_chunk(const BnGeom &g, int N) {
    long nb2 = g.V / ((long)g.R * 8);
    if (nb2 < 1) nb2 = 1;
    long cap2 = 8192 / N > 0 ? 8192 / N : 1;
    if (nb2 > cap2) nb2 = cap2;
    return cdiv(g.V, nb2);
}

// VEC consecutive channels at element e, as fp32
template <int VEC, bool BF>
__device__ __forceinline__ void bn_ld(const void *p, size_t e, float (&f)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 q = ld4<BF>(p, e);
        f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
    } else
        f[0] = ld1<BF>(p, e);
}
template <int VEC, bool BF>
__device__ __forceinline__ void bn_st(void *p, size_t e, const float (&f)[VEC]) {
    if constexpr (VEC == 4)
        st4<BF>(p, e, f[0], f[1], f[2], f[3]);
    else
        st1<BF>(p, e, f[0]);
}

// rows r < R of the block -> partial[(n * nblk + b)][c][2], rows added in ascending order
template <int VEC>
__device__ __forceinline__ void bn_block_reduce(const double (&s)[VEC], const double (&ss)[VEC], double *sm,
                                                double *__restrict__ partial, int C, int R, int g, int r) {
    if (r < R) {
#pragma unroll
        for (int i = 0; i < VEC; i++) {
            sm[((size_t)r * C + g * VEC + i) * 2 + 0] = s[i];
            sm[((size_t)r * C + g * VEC + i) * 2 + 1] = ss[i];
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double a = 0, q = 0;
        for (int rr = 0; rr < R; rr++) {
            a += sm[((size_t)rr * C + c) * 2 + 0];
            q += sm[((size_t)rr * C + c) * 2 + 1];
        }
        const size_t o = (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * C + c) * 2;
        partial[o] = a;
        partial[o + 1] = q;
    }
}

// ---- fwd pass 1: partial[n][b][c][2] = (sum x, sum x^2) in fp64
template <int VEC, bool XB>
__global__ __launch_bounds__(1024) void k_bn_stats(const void *__restrict__ x, double *__restrict__ partial, int C, int CG,
                                                   int R, long V, long chunk) {
    extern __shared__ double sm[];  // [R][C][2]
    const int n = blockIdx.y, t = threadIdx.x;
    const int g = t % CG, r = t / CG;
    const long v0 = (long)blockIdx.x * chunk;
    long v1 = v0 + chunk;
    if (v1 > V) v1 = V;
    double s[VEC], ss[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i++) s[i] = ss[i] = 0.0;
    if (r < R) {
        const size_t base = ((size_t)n * V) * C + (size_t)g * VEC;
        long v = v0 + r;
        for (; v + 3L * R < v1; v += 4L * R) {  // four rows in flight per thread, accumulated in row order
            float f[4][VEC];
#pragma unroll
            for (int u = 0; u < 4; u++) bn_ld<VEC, XB>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
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
            bn_ld<VEC, XB>(x, base + (size_t)v * C, f);
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                s[i] += (double)f[i];
                ss[i] += (double)f[i] * (double)f[i];
            }
        }
    }
    bn_block_reduce<VEC>(s, ss, sm, partial, C, R, g, r);
}

// all `total` = N * nblk block partials of channel c, summed by one wave: lanes stride over them (two in flight), then the
// fixed shuffle tree.  Valid in lane 0.
__device__ __forceinline__ void bn_channel_sum(const double *__restrict__ partial, int C, int c, long total, double &a,
                                               double &q) {
    double a0 = 0, q0 = 0, a1 = 0, q1 = 0;
    long j = threadIdx.x;
    for (; j + 64 < total; j += 128) {
        const size_t o = ((size_t)j * C + c) * 2, o1 = ((size_t)(j + 64) * C + c) * 2;
        const double va = partial[o], vq = partial[o + 1], wa = partial[o1], wq = partial[o1 + 1];
        a0 += va; q0 += vq; a1 += wa; q1 += wq;
    }
    for (; j < total; j += 64) {
        const size_t o = ((size_t)j * C + c) * 2;
        a0 += partial[o];
        q0 += partial[o + 1];
    }
    a = wave_sum(a0 + a1);
    q = wave_sum(q0 + q1);
}

// one wave per channel: mean, rstd (biased variance, formed in fp64, clamped at 0), the running buffers
// (torch.nn.functional.batch_norm: running_var takes the UNBIASED variance) and the step counter
__global__ void k_bn_finalize(const double *__restrict__ partial, float *__restrict__ mean, float *__restrict__ rstd,
                              float *__restrict__ running_mean, float *__restrict__ running_var,
                              long long *__restrict__ num_batches_tracked, int C, long total, long M, float eps,
                              double momentum) {
    const int c = blockIdx.x;
    double a, q;
    bn_channel_sum(partial, C, c, total, a, q);
    if (threadIdx.x != 0) return;
    const double m = a / (double)M;
    double var = q / (double)M - m * m;
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
    const int n = blockIdx.y, t = threadIdx.x;
    const int g = t % CG, r = t / CG;
    if (r >= R) return;
    const long v0 = (long)blockIdx.x * chunk;
    long v1 = v0 + chunk;
    if (v1 > V) v1 = V;
    float mu[VEC], rs[VEC], ga[VEC], be[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i++) {
        const int c = g * VEC + i;
        mu[i] = mean[c];
        rs[i] = EVAL ? (float)(1.0 / sqrt((double)rstd_or_var[c] + (double)eps)) : rstd_or_var[c];
        ga[i] = gamma[c];
        be[i] = beta[c];
    }
    const size_t base = ((size_t)n * V) * C + (size_t)g * VEC;
    long v = v0 + r;
    for (; v + 3L * R < v1; v += 4L * R) {  // four independent rows in flight
        float f[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; u++) bn_ld<VEC, XB>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                const float xh = (f[u][i] - mu[i]) * rs[i];
                const float z = fmaf(xh, ga[i], be[i]);  // (explicit: the same rounding in every kernel that re-computes z)
                f[u][i] = z > 0.f ? z : z * slope;
            }
            bn_st<VEC, YB>(y, base + (size_t)(v + (long)u * R) * C, f[u]);
        }
    }
    for (; v < v1; v += R) {
        float f[VEC];
        bn_ld<VEC, XB>(x, base + (size_t)v * C, f);
#pragma unroll
        for (int i = 0; i < VEC; i++) {
            const float xh = (f[i] - mu[i]) * rs[i];
            const float z = fmaf(xh, ga[i], be[i]);
            f[i] = z > 0.f ? z : z * slope;
        }
        bn_st<VEC, YB>(y, base + (size_t)v * C, f);
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
    const int n = blockIdx.y, t = threadIdx.x;
    const int g = t % CG, r = t / CG;
    const long v0 = (long)blockIdx.x * chunk;
    long v1 = v0 + chunk;
    if (v1 > V) v1 = V;
    double s[VEC], ss[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i++) s[i] = ss[i] = 0.0;
    if (r < R) {
        float mu[VEC], rs[VEC], ga[VEC], be[VEC];
#pragma unroll
        for (int i = 0; i < VEC; i++) {
            const int c = g * VEC + i;
            mu[i] = mean[c];
            rs[i] = rstd[c];
            ga[i] = gamma[c];
            be[i] = beta[c];
        }
        const size_t base = ((size_t)n * V) * C + (size_t)g * VEC;
        long v = v0 + r;
        for (; v + R < v1; v += 2L * R) {  // two rows (four loads) in flight per thread, accumulated in row order
            float f[2][VEC], d[2][VEC];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                bn_ld<VEC, XB>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
                bn_ld<VEC, YB>(dy, base + (size_t)(v + (long)u * R) * C, d[u]);
            }
#pragma unroll
            for (int u = 0; u < 2; u++)
#pragma unroll
                for (int i = 0; i < VEC; i++) {
                    const float xh = (f[u][i] - mu[i]) * rs[i];
                    const float z = fmaf(xh, ga[i], be[i]);
                    const float dz = z > 0.f ? d[u][i] : d[u][i] * slope;
                    s[i] += (double)dz;
                    ss[i] += (double)dz * (double)xh;
                }
        }
        for (; v < v1; v += R) {
            float f[VEC], d[VEC];
            bn_ld<VEC, XB>(x, base + (size_t)v * C, f);
            bn_ld<VEC, YB>(dy, base + (size_t)v * C, d);
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                const float xh = (f[i] - mu[i]) * rs[i];
                const float z = fmaf(xh, ga[i], be[i]);
                const float dz = z > 0.f ? d[i] : d[i] * slope;
                s[i] += (double)dz;
                ss[i] += (double)dz * (double)xh;
            }
        }
    }
    bn_block_reduce<VEC>(s, ss, sm, partial, C, R, g, r);
}

// one wave per channel over all n: sums[c][2] (float) = (sum dz, sum dz * xhat) = (dbeta, dgamma)
__global__ void k_bn_bwd_finalize(const double *__restrict__ partial, float *__restrict__ sums, float *__restrict__ dgamma,
                                  float *__restrict__ dbeta, int C, long total) {
    const int c = blockIdx.x;
    double a, q;
    bn_channel_sum(partial, C, c, total, a, q);
    if (threadIdx.x != 0) return;
    sums[(size_t)c * 2 + 0] = (float)a;
    sums[(size_t)c * 2 + 1] = (float)q;
    dgamma[c] = (float)q;  // (scalar stores: the gradients may be slices of a flat buffer)
    dbeta[c] = (float)a;
}

// ---- bwd pass 2: dx = gamma * rstd * (dz - sum dz / M - xhat * sum dz xhat / M), in x's dtype
template <int VEC, bool XB, bool YB>
__global__ __launch_bounds__(1024) void k_bn_bwd_apply(const void *__restrict__ x, const void *__restrict__ dy,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       const float *__restrict__ mean, const float *__restrict__ rstd,
                                                       const float *__restrict__ sums, void *__restrict__ dx, int C, int CG,
                                                       int R, long V, long chunk, float invM, float slope) {
    const int n = blockIdx.y, t = threadIdx.x;
    const int g = t % CG, r = t / CG;
    if (r >= R) return;
    const long v0 = (long)blockIdx.x * chunk;
    long v1 = v0 + chunk;
    if (v1 > V) v1 = V;
    float mu[VEC], rs[VEC], ga[VEC], be[VEC], m1[VEC], m2[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i++) {
        const int c = g * VEC + i;
        mu[i] = mean[c];
        rs[i] = rstd[c];
        ga[i] = gamma[c];
        be[i] = beta[c];
        m1[i] = sums[(size_t)c * 2 + 0] * invM;
        m2[i] = sums[(size_t)c * 2 + 1] * invM;
    }
    const size_t base = ((size_t)n * V) * C + (size_t)g * VEC;
    long v = v0 + r;
    for (; v + 3L * R < v1; v += 4L * R) {  // four rows (eight loads) in flight
        float f[4][VEC], d[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            bn_ld<VEC, XB>(x, base + (size_t)(v + (long)u * R) * C, f[u]);
            bn_ld<VEC, YB>(dy, base + (size_t)(v + (long)u * R) * C, d[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                const float xh = (f[u][i] - mu[i]) * rs[i];
                const float z = fmaf(xh, ga[i], be[i]);
                const float dz = z > 0.f ? d[u][i] : d[u][i] * slope;
                f[u][i] = ga[i] * rs[i] * (dz - m1[i] - xh * m2[i]);
            }
            bn_st<VEC, XB>(dx, base + (size_t)(v + (long)u * R) * C, f[u]);
        }
    }
    for (; v < v1; v += R) {
        float f[VEC], d[VEC];
        bn_ld<VEC, XB>(x, base + (size_t)v * C, f);
        bn_ld<VEC, YB>(dy, base + (size_t)v * C, d);
#pragma unroll
        for (int i = 0; i < VEC; i++) {
            const float xh = (f[i] - mu[i]) * rs[i];
            const float z = fmaf(xh, ga[i], be[i]);
            const float dz = z > 0.f ? d[i] : d[i] * slope;
            f[i] = ga[i] * rs[i] * (dz - m1[i] - xh * m2[i]);
        }
        bn_st<VEC, XB>(dx, base + (size_t)v * C, f);
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
    const BnGeom g = bn_geom(N, V, C);
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
    const BnGeom g = bn_geom(N, V, C);
    const bool v4 = g.VEC == 4, xb = x_is_bf16 != 0, yb = y_is_bf16 != 0;
    hipStream_t s = as_stream(stream);
    double *partial = reinterpret_cast<double *>(ws);
    const size_t sm = (size_t)g.R * C * 2 * sizeof(double);  // <= 16 KiB for C <= 1024
    auto stats = v4 ? (xb ? k_bn_stats<4, true> : k_bn_stats<4, false>) : (xb ? k_bn_stats<1, true> : k_bn_stats<1, false>);
    hipLaunchKernelGGL(stats, dim3(g.nblk, N), dim3(g.threads), sm, s, x, partial, C, g.CG, g.R, V, g.chunk);
    if (check_launch("batchnorm stats")) return 1;
    hipLaunchKernelGGL(k_bn_finalize, dim3(C), dim3(64), 0, s, partial, mean, rstd, running_mean, running_var,
                       reinterpret_cast<long long *>(num_batches_tracked), C, (long)N * g.nblk, (long)N * V, eps, momentum);
    if (check_launch("batchnorm finalize")) return 1;
    const long chunk2 = bn_apply_chunk(g, N);
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
    const BnGeom g = bn_geom(N, V, C);
    const bool v4 = g.VEC == 4, xb = x_is_bf16 != 0, yb = y_is_bf16 != 0;
    const long chunk2 = bn_apply_chunk(g, N);
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
    const BnGeom g = bn_geom(N, V, C);
    const bool v4 = g.VEC == 4, xb = x_is_bf16 != 0, yb = y_is_bf16 != 0;
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
    const long chunk2 = bn_apply_chunk(g, N);
    auto apply = MVD_BN_PICK(k_bn_bwd_apply, v4, xb, yb);
    hipLaunchKernelGGL(apply, dim3((unsigned)cdiv(V, chunk2), N), dim3(g.threads), 0, s, x, dy, gamma, beta, mean, rstd, sums, dx,
                       C, g.CG, g.R, V, chunk2, (float)(1.0 / (double)((long)N * V)), slope);
    return check_launch("batchnorm bwd apply");
}
}
