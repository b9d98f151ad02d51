// The tail of a residual block (BasicBlockD of the residual-encoder U-Net) and the average pool of its skip branch, fp32 on
// NDHWC activations [N,V,C].
//   forward   y = lrelu( IN(a) * gamma_a + beta_a + R ),  R = r (identity / pool-only skip) or IN(r) * gamma_r + beta_r (the
//             1x1x1 projection skip, normalised in the same pass: the normalised skip tensor is never written)
//   backward  g = dy * lrelu'(z) with z re-computed by the forward's arithmetic (rb_z below, one function for both passes);
//             da = InstanceNorm backward of g through a; dr = g (identity form) or InstanceNorm backward of g through r
// HBM-bound.  Identity form: forward = read a (statistics) + read a, r + write y; backward = read a, r, dy (sums) + read a,
// r, dy + write da, dr.  Geometry, row walk and statistics are those of norm_common.h, shared with instnorm.hip and
// batchnorm.hip: per-thread fp64 accumulation in row order -> fixed-order LDS reduce -> per-block partials -> fixed-order
// finalize (one wave per channel, fixed shuffle tree).  No atomics anywhere: a graph replay repeats the eager step bit
// for bit.
#include "norm_common.h"

namespace mvd {

// per-channel constants of one thread
template <int VEC, bool PROJ>
struct RbCh {
    float mu[VEC], rs[VEC], ga[VEC], be[VEC], mur[VEC], rsr[VEC], gr[VEC], br[VEC];
    __device__ __forceinline__ void load(int n, int C, int c0, const float *mean_a, const float *rstd_a, const float *gamma_a,
                                         const float *beta_a, const float *mean_r, const float *rstd_r, const float *gamma_r,
                                         const float *beta_r) {
        norm_consts<VEC>(mu, rs, ga, be, mean_a, rstd_a, gamma_a, beta_a, (size_t)n * C, c0);
        if (PROJ)
            norm_consts<VEC>(mur, rsr, gr, br, mean_r, rstd_r, gamma_r, beta_r, (size_t)n * C, c0);
        else
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                mur[i] = 0.f; rsr[i] = 1.f; gr[i] = 1.f; br[i] = 0.f;
            }
    }
};

// the pre-activation of the block tail, channel i of the thread: norm_z of a, plus r or norm_z of r; xa / xr return the
// normalised values
template <int VEC, bool PROJ>
__device__ __forceinline__ float rb_z(const RbCh<VEC, PROJ> &ch, int i, float a, float r, float &xa, float &xr) {
    const float za = norm_z(a, ch.mu[i], ch.rs[i], ch.ga[i], ch.be[i], xa);
    if (PROJ) return za + norm_z(r, ch.mur[i], ch.rsr[i], ch.gr[i], ch.br[i], xr);
    xr = 0.f;
    return za + r;
}

// ---- forward pass 1: partial[t][n][b][c][2] = (sum x, sum x^2) in fp64 of tensor t = blockIdx.z (0: a, 1: r)
template <int VEC>
__global__ void k_rb_stats(const float *__restrict__ a, const float *__restrict__ r_, double *__restrict__ partial, int C, int CG,
                           int R, long V, long chunk) {
    extern __shared__ double sm[];  // [R][C][2]
    const NormThread<VEC> t(CG, V, chunk);
    if (t.r < R) {
        double s[VEC] = {}, ss[VEC] = {};
        norm_moments<VEC, false>(blockIdx.z ? r_ : a, t.base(V, C), t.v0 + t.r, t.v1, R, C, s, ss);
        norm_row_store<VEC>(sm, C, t.c0(), t.r, s, ss);
    }
    norm_block_reduce<2>(sm, partial, C, R, ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
}

// one wave per (c, n, tensor): lanes stride over the block partials, fixed shuffle tree; biased variance, eps inside the root
__global__ void k_rb_finalize(const double *__restrict__ partial, float *__restrict__ mean_a, float *__restrict__ rstd_a,
                              float *__restrict__ mean_r, float *__restrict__ rstd_r, int C, int nblk, long V, float eps) {
    const int c = blockIdx.x, n = blockIdx.y, N = gridDim.y;
    double s[2];
    norm_wave_sum<2>(partial, C, c, ((size_t)blockIdx.z * N + n) * nblk, nblk, s);
    if (threadIdx.x != 0) return;
    const double m = s[0] / (double)V;
    double var = s[1] / (double)V - m * m;
    if (var < 0) var = 0;
    float *mean = blockIdx.z ? mean_r : mean_a, *rstd = blockIdx.z ? rstd_r : rstd_a;
    mean[(size_t)n * C + c] = (float)m;
    rstd[(size_t)n * C + c] = (float)(1.0 / sqrt(var + (double)eps));
}

// ---- forward pass 2
template <int VEC, bool PROJ>
__global__ void k_rb_apply(const float *__restrict__ a, const float *__restrict__ r_, const float *__restrict__ gamma_a,
                           const float *__restrict__ beta_a, const float *__restrict__ mean_a, const float *__restrict__ rstd_a,
                           const float *__restrict__ gamma_r, const float *__restrict__ beta_r, const float *__restrict__ mean_r,
                           const float *__restrict__ rstd_r, float *__restrict__ y, int C, int CG, int R, long V, long chunk,
                           float slope) {
    const int n = blockIdx.y;
    const NormThread<VEC> t(CG, V, chunk);
    if (t.r >= R) return;
    const size_t base = t.base(V, C);
    RbCh<VEC, PROJ> ch;
    ch.load(n, C, t.c0(), mean_a, rstd_a, gamma_a, beta_a, mean_r, rstd_r, gamma_r, beta_r);
    long v = t.v0 + t.r;
    for (; v + (long)R < t.v1; v += 2L * R) {  // two rows of both tensors in flight
        float fa[2][VEC], fr[2][VEC];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            norm_ld<VEC, false>(a, base + (size_t)(v + (long)u * R) * C, fa[u]);
            norm_ld<VEC, false>(r_, base + (size_t)(v + (long)u * R) * C, fr[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                float xa, xr;
                const float z = rb_z(ch, i, fa[u][i], fr[u][i], xa, xr);
                fa[u][i] = z > 0.f ? z : z * slope;
            }
            norm_st<VEC, false>(y, base + (size_t)(v + (long)u * R) * C, fa[u]);
        }
    }
    for (; v < t.v1; v += R) {
        float fa[VEC], fr[VEC];
        norm_ld<VEC, false>(a, base + (size_t)v * C, fa);
        norm_ld<VEC, false>(r_, base + (size_t)v * C, fr);
#pragma unroll
        for (int i = 0; i < VEC; i++) {
            float xa, xr;
            const float z = rb_z(ch, i, fa[i], fr[i], xa, xr);
            fa[i] = z > 0.f ? z : z * slope;
        }
        norm_st<VEC, false>(y, base + (size_t)v * C, fa);
    }
}

// ---- backward pass 1: partial[n][b][c][NS] = (sum g, sum g*xhat_a[, sum g*xhat_r]) in fp64, g = dy * lrelu'(z)
template <int VEC, bool PROJ>
__global__ void k_rb_bwd_stats(const float *__restrict__ a, const float *__restrict__ r_, const float *__restrict__ dy,
                               const float *__restrict__ gamma_a, const float *__restrict__ beta_a,
                               const float *__restrict__ mean_a, const float *__restrict__ rstd_a,
                               const float *__restrict__ gamma_r, const float *__restrict__ beta_r,
                               const float *__restrict__ mean_r, const float *__restrict__ rstd_r, double *__restrict__ partial,
                               int C, int CG, int R, long V, long chunk, float slope) {
    constexpr int NS = PROJ ? 3 : 2;
    extern __shared__ double sm[];  // [R][C][NS]
    const int n = blockIdx.y;
    const NormThread<VEC> t(CG, V, chunk);
    if (t.r < R) {
        double s1[VEC] = {}, s2[VEC] = {}, s3[VEC] = {};
        const size_t base = t.base(V, C);
        RbCh<VEC, PROJ> ch;
        ch.load(n, C, t.c0(), mean_a, rstd_a, gamma_a, beta_a, mean_r, rstd_r, gamma_r, beta_r);
        long v = t.v0 + t.r;
        for (; v + (long)R < t.v1; v += 2L * R) {  // two rows of the three tensors in flight, accumulated in row order
            float fa[2][VEC], fr[2][VEC], fd[2][VEC];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                norm_ld<VEC, false>(a, base + (size_t)(v + (long)u * R) * C, fa[u]);
                norm_ld<VEC, false>(r_, base + (size_t)(v + (long)u * R) * C, fr[u]);
                norm_ld<VEC, false>(dy, base + (size_t)(v + (long)u * R) * C, fd[u]);
            }
#pragma unroll
            for (int u = 0; u < 2; u++)
#pragma unroll
                for (int i = 0; i < VEC; i++) {
                    float xa, xr;
                    const float z = rb_z(ch, i, fa[u][i], fr[u][i], xa, xr);
                    const float gz = z > 0.f ? fd[u][i] : fd[u][i] * slope;
                    s1[i] += (double)gz;
                    s2[i] += (double)gz * (double)xa;
                    if (PROJ) s3[i] += (double)gz * (double)xr;
                }
        }
        for (; v < t.v1; v += R) {
            float fa[VEC], fr[VEC], fd[VEC];
            norm_ld<VEC, false>(a, base + (size_t)v * C, fa);
            norm_ld<VEC, false>(r_, base + (size_t)v * C, fr);
            norm_ld<VEC, false>(dy, base + (size_t)v * C, fd);
#pragma unroll
            for (int i = 0; i < VEC; i++) {
                float xa, xr;
                const float z = rb_z(ch, i, fa[i], fr[i], xa, xr);
                const float gz = z > 0.f ? fd[i] : fd[i] * slope;
                s1[i] += (double)gz;
                s2[i] += (double)gz * (double)xa;
                if (PROJ) s3[i] += (double)gz * (double)xr;
            }
        }
        if constexpr (PROJ)
            norm_row_store<VEC>(sm, C, t.c0(), t.r, s1, s2, s3);
        else
            norm_row_store<VEC>(sm, C, t.c0(), t.r, s1, s2);
    }
    norm_block_reduce<NS>(sm, partial, C, R, (size_t)n * gridDim.x + blockIdx.x);
}

// sums[n][c][NS] (float); dgamma / dbeta over n in ascending order.  One wave per channel.
template <bool PROJ>
__global__ void k_rb_bwd_finalize(const double *__restrict__ partial, float *__restrict__ sums, float *__restrict__ dgamma_a,
                                  float *__restrict__ dbeta_a, float *__restrict__ dgamma_r, float *__restrict__ dbeta_r, int N,
                                  int C, int nblk) {
    constexpr int NS = PROJ ? 3 : 2;
    const int c = blockIdx.x;
    double tot[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) tot[k] = 0;
    for (int n = 0; n < N; n++) {
        double q[NS];
        norm_wave_sum<NS>(partial, C, c, (size_t)n * nblk, nblk, q);
#pragma unroll
        for (int k = 0; k < NS; k++) {
            if (threadIdx.x == 0) sums[((size_t)n * C + c) * NS + k] = (float)q[k];
            tot[k] += q[k];
        }
    }
    if (threadIdx.x == 0) {
        dbeta_a[c] = (float)tot[0];
        dgamma_a[c] = (float)tot[1];
        if (PROJ) {
            dbeta_r[c] = (float)tot[0];  // beta_r enters z as beta_a does
            dgamma_r[c] = (float)tot[2];
        }
    }
}

// ---- backward pass 2
template <int VEC, bool PROJ>
__global__ void k_rb_bwd_apply(const float *__restrict__ a, const float *__restrict__ r_, const float *__restrict__ dy,
                               const float *__restrict__ gamma_a, const float *__restrict__ beta_a,
                               const float *__restrict__ mean_a, const float *__restrict__ rstd_a,
                               const float *__restrict__ gamma_r, const float *__restrict__ beta_r,
                               const float *__restrict__ mean_r, const float *__restrict__ rstd_r, const float *__restrict__ sums,
                               float *__restrict__ da, float *dr, int accumulate, int C, int CG, int R, long V, long chunk,
                               float slope) {
    constexpr int NS = PROJ ? 3 : 2;
    const int n = blockIdx.y;
    const NormThread<VEC> t(CG, V, chunk);
    if (t.r >= R) return;
    const size_t base = t.base(V, C);
    RbCh<VEC, PROJ> ch;
    ch.load(n, C, t.c0(), mean_a, rstd_a, gamma_a, beta_a, mean_r, rstd_r, gamma_r, beta_r);
    const float invV = 1.0f / (float)V;
    float m1[VEC], m2[VEC], m3[VEC], ka[VEC], kr[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i++) {
        const size_t o = ((size_t)n * C + t.c0() + i) * NS;
        m1[i] = sums[o] * invV;
        m2[i] = sums[o + 1] * invV;
        m3[i] = PROJ ? sums[o + 2] * invV : 0.f;
        ka[i] = ch.ga[i] * ch.rs[i];
        kr[i] = ch.gr[i] * ch.rsr[i];
    }
    for (long v = t.v0 + t.r; v < t.v1; v += R) {
        const size_t e = base + (size_t)v * C;
        float fa[VEC], fr[VEC], fd[VEC], fo[VEC];
        norm_ld<VEC, false>(a, e, fa);
        norm_ld<VEC, false>(r_, e, fr);
        norm_ld<VEC, false>(dy, e, fd);
        if (accumulate) norm_ld<VEC, false>(dr, e, fo);
#pragma unroll
        for (int i = 0; i < VEC; i++) {
            float xa, xr;
            const float z = rb_z(ch, i, fa[i], fr[i], xa, xr);
            const float gz = z > 0.f ? fd[i] : fd[i] * slope;
            fa[i] = ka[i] * (gz - m1[i] - xa * m2[i]);
            const float d = PROJ ? kr[i] * (gz - m1[i] - xr * m3[i]) : gz;
            fr[i] = accumulate ? fo[i] + d : d;
        }
        norm_st<VEC, false>(da, e, fa);
        norm_st<VEC, false>(dr, e, fr);
    }
}

// ---- average pool, kernel = stride, NDHWC.  The taps are added in (z, y, x) order and scaled by 1 / count (a power of
// two: one rounding, the value of torch's sum / count).
template <int VEC>
__global__ void k_avgpool_fwd(const float *__restrict__ x, float *__restrict__ y, long total, int C, int D, int H, int W, int od,
                              int oh, int ow, int sd, int sh, int sw) {
    const int CG = C / VEC;
    const float inv = 1.0f / (float)(sd * sh * sw);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int g = (int)(i % CG);
        long p = i / CG;
        const int xo = (int)(p % ow);
        p /= ow;
        const int yo = (int)(p % oh);
        p /= oh;
        const int zo = (int)(p % od);
        const long n = p / od;
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; k++) acc[k] = 0.f;
        for (int dz = 0; dz < sd; dz++)
            for (int dyy = 0; dyy < sh; dyy++)
                for (int dx = 0; dx < sw; dx++) {
                    const size_t e =
                        ((((size_t)n * D + (zo * sd + dz)) * H + (yo * sh + dyy)) * W + (xo * sw + dx)) * C + (size_t)g * VEC;
                    float f[VEC];
                    norm_ld<VEC, false>(x, e, f);
#pragma unroll
                    for (int k = 0; k < VEC; k++) acc[k] += f[k];
                }
#pragma unroll
        for (int k = 0; k < VEC; k++) acc[k] *= inv;
        norm_st<VEC, false>(y, (size_t)i * VEC, acc);
    }
}

// thread = VEC channels of one INPUT voxel: dx = dy[its window] / count (+ dx when accumulating)
template <int VEC>
__global__ void k_avgpool_bwd(const float *__restrict__ dy, float *dx, long total, int C, int D, int H, int W, int od, int oh,
                              int ow, int sd, int sh, int sw, int accumulate) {
    const int CG = C / VEC;
    const float inv = 1.0f / (float)(sd * sh * sw);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int g = (int)(i % CG);
        long p = i / CG;
        const int xi = (int)(p % W);
        p /= W;
        const int yi = (int)(p % H);
        p /= H;
        const int zi = (int)(p % D);
        const long n = p / D;
        const size_t e = ((((size_t)n * od + zi / sd) * oh + yi / sh) * ow + xi / sw) * C + (size_t)g * VEC;
        float f[VEC], o[VEC];
        norm_ld<VEC, false>(dy, e, f);
        if (accumulate) norm_ld<VEC, false>(dx, (size_t)i * VEC, o);
#pragma unroll
        for (int k = 0; k < VEC; k++) f[k] = accumulate ? o[k] + f[k] * inv : f[k] * inv;
        norm_st<VEC, false>(dx, (size_t)i * VEC, f);
    }
}

static bool rb_aligned(const void *p, int C) { return C % 4 != 0 || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int rb_shape_ok(const char *who, int N, long V, int C) {
    MVD_REQUIRE(N > 0 && V > 0 && C > 0, "%s: N, V and C must be positive (got %d, %ld, %d)", who, N, V, C);
    MVD_REQUIRE(V > 1, "%s: InstanceNorm needs more than 1 spatial element per channel", who);
    MVD_REQUIRE(N <= 65535 && C <= 1024, "%s: N <= 65535 and C <= 1024 (got %d, %d)", who, N, C);
    return 0;
}

static int pool_shape_ok(const char *who, int N, int C, int D, int H, int W, const int stride[3]) {
    MVD_REQUIRE(stride, "%s: null stride", who);
    MVD_REQUIRE(N > 0 && C > 0 && D > 0 && H > 0 && W > 0, "%s: N, C and the extents must be positive", who);
    const int ext[3] = {D, H, W};
    for (int i = 0; i < 3; i++) {
        MVD_REQUIRE(stride[i] == 1 || stride[i] == 2, "%s: stride 1 or 2 per axis (got %d)", who, stride[i]);
        MVD_REQUIRE(ext[i] % stride[i] == 0,
                    "%s: odd extent %d on a strided axis (the pool floors where the strided conv beside it does not)", who,
                    ext[i]);
    }
    return 0;
}

static unsigned pool_grid(long total) {
    long g = cdiv(total, 256);
    if (g > (1L << 20)) g = 1L << 20;
    return (unsigned)g;
}

}  // namespace mvd

using namespace mvd;

extern "C" {

size_t mvd_resblock_workspace_bytes(int N, long V, int C) {
    if (N <= 0 || V <= 0 || C <= 0) return 256;
    const NormGeom g = norm_geom(N, V, C);
    // block partials: 2 tensors x 2 sums (forward) or 3 sums (backward) -> 4 doubles; then sums [N][C][3] floats
    return (size_t)N * g.nblk * C * 4 * sizeof(double) + (size_t)N * C * 3 * sizeof(float) + 256;
}

int mvd_resblock_fwd(const float *a, const float *gamma_a, const float *beta_a, const float *r, const float *gamma_r,
                     const float *beta_r, float *y, float *mean_a, float *rstd_a, float *mean_r, float *rstd_r, int N, long V,
                     int C, float eps, float slope, int have_stats, void *ws, size_t ws_bytes, void *stream) {
    if (const int rc = rb_shape_ok("resblock_fwd", N, V, C)) return rc;
    const bool proj = gamma_r != nullptr;
    MVD_REQUIRE(a && gamma_a && beta_a && r && y && mean_a && rstd_a && ws, "resblock_fwd: null pointer");
    MVD_REQUIRE(!proj || (beta_r && mean_r && rstd_r), "resblock_fwd: the projection form needs beta_r, mean_r and rstd_r");
    MVD_REQUIRE(ws_bytes >= mvd_resblock_workspace_bytes(N, V, C), "resblock_fwd: workspace too small");
    MVD_REQUIRE(rb_aligned(a, C) && rb_aligned(r, C) && rb_aligned(y, C),
                "resblock_fwd: a, r and y must be 16-byte aligned for C %% 4 == 0");
    hipStream_t s = as_stream(stream);
    const NormGeom g = norm_geom(N, V, C);
    double *partial = reinterpret_cast<double *>(ws);
    // have_stats: bit 0 mean_a / rstd_a, bit 1 mean_r / rstd_r are already filled (mvd_instnorm_stats_from_tiles)
    const bool need_a = !(have_stats & 1), need_r = proj && !(have_stats & 2);
    if (need_a || need_r) {
        const float *t0 = need_a ? a : r;
        const int nz = (need_a && need_r) ? 2 : 1;
        const size_t lds = (size_t)g.R * C * 2 * sizeof(double);
        if (g.vec == 4)
            hipLaunchKernelGGL(k_rb_stats<4>, dim3(g.nblk, N, nz), dim3(g.threads), lds, s, t0, r, partial, C, g.CG, g.R, V,
                               g.chunk);
        else
            hipLaunchKernelGGL(k_rb_stats<1>, dim3(g.nblk, N, nz), dim3(g.threads), lds, s, t0, r, partial, C, g.CG, g.R, V,
                               g.chunk);
        if (check_launch("resblock stats")) return 1;
        hipLaunchKernelGGL(k_rb_finalize, dim3(C, N, nz), dim3(64), 0, s, partial, need_a ? mean_a : mean_r,
                           need_a ? rstd_a : rstd_r, mean_r, rstd_r, C, g.nblk, V, eps);
        if (check_launch("resblock finalize")) return 1;
    }
    const long achunk = norm_apply_chunk(g, 65535);  // (the cap: grid.x)
    const dim3 agrid((unsigned)cdiv(V, achunk), N);
#define MVD_RB_APPLY(VV, PP)                                                                                                   \
    hipLaunchKernelGGL((k_rb_apply<VV, PP>), agrid, dim3(g.threads), 0, s, a, r, gamma_a, beta_a, mean_a, rstd_a, gamma_r, beta_r, \
                       mean_r, rstd_r, y, C, g.CG, g.R, V, achunk, slope)
    if (g.vec == 4) {
        if (proj) MVD_RB_APPLY(4, true); else MVD_RB_APPLY(4, false);
    } else {
        if (proj) MVD_RB_APPLY(1, true); else MVD_RB_APPLY(1, false);
    }
#undef MVD_RB_APPLY
    return check_launch("resblock apply");
}

int mvd_resblock_bwd(const float *a, const float *r, const float *dy, const float *gamma_a, const float *beta_a,
                     const float *mean_a, const float *rstd_a, const float *gamma_r, const float *beta_r, const float *mean_r,
                     const float *rstd_r, float *da, float *dr, float *dgamma_a, float *dbeta_a, float *dgamma_r, float *dbeta_r,
                     int accumulate, int N, long V, int C, float slope, void *ws, size_t ws_bytes, void *stream) {
    if (const int rc = rb_shape_ok("resblock_bwd", N, V, C)) return rc;
    const bool proj = gamma_r != nullptr;
    MVD_REQUIRE(a && r && dy && gamma_a && beta_a && mean_a && rstd_a && da && dr && dgamma_a && dbeta_a && ws,
                "resblock_bwd: null pointer");
    MVD_REQUIRE(!proj || (beta_r && mean_r && rstd_r && dgamma_r && dbeta_r),
                "resblock_bwd: the projection form needs beta_r, mean_r, rstd_r, dgamma_r and dbeta_r");
    MVD_REQUIRE(ws_bytes >= mvd_resblock_workspace_bytes(N, V, C), "resblock_bwd: workspace too small");
    MVD_REQUIRE(rb_aligned(a, C) && rb_aligned(r, C) && rb_aligned(dy, C) && rb_aligned(da, C) && rb_aligned(dr, C),
                "resblock_bwd: a, r, dy, da and dr must be 16-byte aligned for C %% 4 == 0");
    hipStream_t s = as_stream(stream);
    const NormGeom g = norm_geom(N, V, C);
    double *partial = reinterpret_cast<double *>(ws);
    float *sums = reinterpret_cast<float *>(partial + (size_t)N * g.nblk * C * 4);
    const long achunk = norm_apply_chunk(g, 65535);
    const dim3 grid(g.nblk, N), agrid((unsigned)cdiv(V, achunk), N);
    const size_t lds = (size_t)g.R * C * (proj ? 3 : 2) * sizeof(double);
#define MVD_RB_BSTATS(VV, PP)                                                                                                  \
    hipLaunchKernelGGL((k_rb_bwd_stats<VV, PP>), grid, dim3(g.threads), lds, s, a, r, dy, gamma_a, beta_a, mean_a, rstd_a,     \
                       gamma_r, beta_r, mean_r, rstd_r, partial, C, g.CG, g.R, V, g.chunk, slope)
    if (g.vec == 4) {
        if (proj) MVD_RB_BSTATS(4, true); else MVD_RB_BSTATS(4, false);
    } else {
        if (proj) MVD_RB_BSTATS(1, true); else MVD_RB_BSTATS(1, false);
    }
#undef MVD_RB_BSTATS
    if (check_launch("resblock bwd stats")) return 1;
    if (proj)
        hipLaunchKernelGGL(k_rb_bwd_finalize<true>, dim3(C), dim3(64), 0, s, partial, sums, dgamma_a, dbeta_a, dgamma_r, dbeta_r,
                           N, C, g.nblk);
    else
        hipLaunchKernelGGL(k_rb_bwd_finalize<false>, dim3(C), dim3(64), 0, s, partial, sums, dgamma_a, dbeta_a, dgamma_r, dbeta_r,
                           N, C, g.nblk);
    if (check_launch("resblock bwd finalize")) return 1;
#define MVD_RB_BAPPLY(VV, PP)                                                                                                  \
    hipLaunchKernelGGL((k_rb_bwd_apply<VV, PP>), agrid, dim3(g.threads), 0, s, a, r, dy, gamma_a, beta_a, mean_a, rstd_a,      \
                       gamma_r, beta_r, mean_r, rstd_r, sums, da, dr, accumulate ? 1 : 0, C, g.CG, g.R, V, achunk, slope)
    if (g.vec == 4) {
        if (proj) MVD_RB_BAPPLY(4, true); else MVD_RB_BAPPLY(4, false);
    } else {
        if (proj) MVD_RB_BAPPLY(1, true); else MVD_RB_BAPPLY(1, false);
    }
#undef MVD_RB_BAPPLY
    return check_launch("resblock bwd apply");
}

int mvd_avgpool3d_fwd(const float *x, float *y, int N, int D, int H, int W, int C, const int stride[3], void *stream) {
    if (const int rc = pool_shape_ok("avgpool3d_fwd", N, C, D, H, W, stride)) return rc;
    MVD_REQUIRE(x && y, "avgpool3d_fwd: null pointer");
    MVD_REQUIRE(rb_aligned(x, C) && rb_aligned(y, C), "avgpool3d_fwd: x and y must be 16-byte aligned for C %% 4 == 0");
    hipStream_t s = as_stream(stream);
    const int od = D / stride[0], oh = H / stride[1], ow = W / stride[2];
    const int vec = C % 4 == 0 ? 4 : 1;
    const long total = (long)N * od * oh * ow * (C / vec);
    if (vec == 4)
        hipLaunchKernelGGL(k_avgpool_fwd<4>, dim3(pool_grid(total)), dim3(256), 0, s, x, y, total, C, D, H, W, od, oh, ow, stride[0],
                           stride[1], stride[2]);
    else
        hipLaunchKernelGGL(k_avgpool_fwd<1>, dim3(pool_grid(total)), dim3(256), 0, s, x, y, total, C, D, H, W, od, oh, ow, stride[0],
                           stride[1], stride[2]);
    return check_launch("avgpool3d forward");
}

int mvd_avgpool3d_bwd(const float *dy, float *dx, int N, int D, int H, int W, int C, const int stride[3], int accumulate,
                      void *stream) {
    if (const int rc = pool_shape_ok("avgpool3d_bwd", N, C, D, H, W, stride)) return rc;
    MVD_REQUIRE(dy && dx, "avgpool3d_bwd: null pointer");
    MVD_REQUIRE(rb_aligned(dy, C) && rb_aligned(dx, C), "avgpool3d_bwd: dy and dx must be 16-byte aligned for C %% 4 == 0");
    hipStream_t s = as_stream(stream);
    const int od = D / stride[0], oh = H / stride[1], ow = W / stride[2];
    const int vec = C % 4 == 0 ? 4 : 1;
    const long total = (long)N * D * H * W * (C / vec);
    if (vec == 4)
        hipLaunchKernelGGL(k_avgpool_bwd<4>, dim3(pool_grid(total)), dim3(256), 0, s, dy, dx, total, C, D, H, W, od, oh, ow,
                           stride[0], stride[1], stride[2], accumulate ? 1 : 0);
    else
        hipLaunchKernelGGL(k_avgpool_bwd<1>, dim3(pool_grid(total)), dim3(256), 0, s, dy, dx, total, C, D, H, W, od, oh, ow,
                           stride[0], stride[1], stride[2], accumulate ? 1 : 0);
    return check_launch("avgpool3d backward");
}

}  // extern "C"
