// The bottleneck fusion block of FinalNetv2 (selfattnNet.py:917-939): LayerNorm over the last axis, token linears,
// multi-head attention and dropout, forward and backward, fp32.
//
//   k_dropout_tick      t += 1 in the device state {seed, t} (one thread, at the head of a training-mode forward)
//   k_dropout_mask      the keep mask of (seed, t, site) as bytes (tests)
//   k_layernorm_fwd     [xs = x + pos;] y = LayerNorm(xs): one wave per row, mean then centred second moment (two passes)
//   k_layernorm_bwd     dx (+ up to two residual gradients, + a dropout-masked copy), dgamma, dbeta, dpos in ONE launch
//   k_gemm              D[I,J] = A[I,K] B[K,J] on v_mfma_f32_16x16x4_f32 through strided, bounds-checked loaders: the token
//                       linear's forward (bias + dropout + residual in the epilogue), input gradient and weight gradient
//                       (+ bias gradient) are three calls of it
//   k_attn_fwd          16 query rows of one (batch, head) per block: S = q k^T on the MFMA into LDS, softmax with the row
//                       maximum subtracted, dropout, O = P v on the MFMA, "+ residual" in the store
//   k_attn_bwd_q        the same block shape: recomputes P from q, k and the saved row maximum / sum, dP = dO v^T,
//                       delta = sum_j P dP, dS, dq = dS k
//   k_attn_bwd_kv       16 key rows per block, all queries: recomputes P^T, dk = dS^T q, dv = P^T dO
//
// q, k and v are read in place from the [B, N, 3C] output of the qkv linear (channel = which C + head dh + j, the reference's
// reshape(B, N, 3, heads, dh)), gradients are written into the same layout: no permuted copies.  No atomics: every output
// element has one writer and every sum one fixed order, so results are bit-identical run to run.
//
// Dropout: element e of site s at step t is kept iff the 24-bit uniform (w >> 40) 2^-24 >= p, w = word e & 3 of
// Philox4x64-10 with key (seed, s) and counter ((e >> 2) + 1, t, 0, 0); kept values are scaled by 1 / (1 - p).  seed and t
// are read from device memory by every kernel, so a replayed graph sees t advance.
#include "common.h"

namespace mvd {

typedef float f32x4a __attribute__((ext_vector_type(4)));

enum { AT_TQ = 16, AT_NMAX = 256, AT_PITCH = AT_NMAX + 4 };   // rows per block, token cap, LDS row pitch (conflict-free A reads)

// ------------------------------------------------------------------------------------------------ dropout
__device__ __forceinline__ bool drop_keep(unsigned long long seed, unsigned long long site, unsigned long long t,
                                          unsigned long long e, float p) {
    unsigned long long w[4];
    philox4x64_10((e >> 2) + 1ull, t, seed, site, w);
    const unsigned j = (unsigned)(e & 3ull);
    const unsigned long long x = j == 0 ? w[0] : j == 1 ? w[1] : j == 2 ? w[2] : w[3];
    return (float)(unsigned)(x >> 40) * 5.9604644775390625e-8f >= p;
}

struct Drop {
    unsigned long long seed, t, site;
    float p, scale;
    __device__ __forceinline__ Drop(const long long *state, float p_, int site_) : seed(0), t(0), site(site_), p(p_), scale(1.f) {
        if (p > 0.f) {
            seed = (unsigned long long)state[0];
            t = (unsigned long long)state[1];
            scale = 1.f / (1.f - p);
        }
    }
    // the factor of element e: 0 or 1 / (1 - p); 1 without dropout
    __device__ __forceinline__ float operator()(unsigned long long e) const {
        if (!(p > 0.f)) return 1.f;
        return drop_keep(seed, site, t, e, p) ? scale : 0.f;
    }
};

__global__ void k_dropout_tick(long long *__restrict__ state) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[1] = state[1] + 1;
}

__global__ void __launch_bounds__(256) k_dropout_mask(unsigned long long seed, unsigned long long t, int site, float p, long n,
                                                      unsigned char *__restrict__ out) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x)
        out[e] = drop_keep(seed, (unsigned long long)site, t, (unsigned long long)e, p) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ helpers
__device__ __forceinline__ float wave_allsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave: the 16 x 16 tile sum_k a(i, k) b(k, j), k < K rounded up to 16 (the loaders return 0 out of range).
// Lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; result register r is D[4 (l >> 4) + r][l & 15].
// Four accumulators take the k steps in turn (independent MFMAs back to back, four times shorter rounding chains) and
// are added pairwise at the end: a fixed order.
template <class FA, class FB>
__device__ __forceinline__ f32x4a mma_tile(int K, FA a, FB b) {
    f32x4a acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const int r = threadIdx.x & 15, kq = (threadIdx.x & 63) >> 4;
    for (int k0 = 0; k0 < K; k0 += 16) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 4 * u + kq;
            acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a(r, k), b(k, r), acc[u], 0, 0, 0);
        }
    }
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// ------------------------------------------------------------------------------------------------ LayerNorm
__global__ void __launch_bounds__(256) k_layernorm_fwd(const float *__restrict__ x, const float *__restrict__ pos,
                                                       float *__restrict__ xs, float *__restrict__ y,
                                                       float *__restrict__ mean_o, float *__restrict__ rstd_o,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       long M, int C, long Npos, float eps) {
    const int lane = threadIdx.x & 63;
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const float *xr = x + m * C;
    const float *pr = pos ? pos + (m % Npos) * C : nullptr;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = pr ? xr[c] + pr[c] : xr[c];
        if (xs) xs[m * C + c] = v;
        s += v;
    }
    const float mean = wave_allsum(s) / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float d = (pr ? xr[c] + pr[c] : xr[c]) - mean;
        q += d * d;
    }
    const float rstd = 1.f / sqrtf(wave_allsum(q) / (float)C + eps);
    for (int c = lane; c < C; c += 64) {
        const float v = pr ? xr[c] + pr[c] : xr[c];
        y[m * C + c] = (v - mean) * rstd * gamma[c] + beta[c];
    }
    if (lane == 0) {
        mean_o[m] = mean;
        rstd_o[m] = rstd;
    }
}

// Rows are viewed [Bv, Nv, C]: with a position embedding Bv is the batch (dpos sums over it), else Bv = 1.  Blocks
// [0, nrow): one wave per token n, its Bv rows in turn.  Blocks [nrow, ...): 64 columns each, dgamma / dbeta over all rows
// in four interleaved row phases that thread 0..63 adds up in a fixed order.
__global__ void __launch_bounds__(256) k_layernorm_bwd(const float *__restrict__ dy, const float *__restrict__ xs,
                                                       const float *__restrict__ mean_i, const float *__restrict__ rstd_i,
                                                       const float *__restrict__ gamma, const float *__restrict__ dres1,
                                                       const float *__restrict__ dres2, float *__restrict__ dx,
                                                       float *__restrict__ dxd, float *__restrict__ dgamma,
                                                       float *__restrict__ dbeta, float *__restrict__ dpos, int Bv, long Nv,
                                                       int C, int nrow, const long long *__restrict__ state, float p,
                                                       int site) {
    __shared__ float sh[4][2][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if ((int)blockIdx.x >= nrow) {
        const int c = ((int)blockIdx.x - nrow) * 64 + lane;
        const long M = (long)Bv * Nv;
        float dg = 0.f, db = 0.f;
        if (c < C)
            for (long m = w; m < M; m += 4) {
                const float g = dy[m * C + c];
                dg += g * ((xs[m * C + c] - mean_i[m]) * rstd_i[m]);
                db += g;
            }
        sh[w][0][lane] = dg;
        sh[w][1][lane] = db;
        __syncthreads();
        if (w == 0 && c < C) {
            dgamma[c] = ((sh[0][0][lane] + sh[1][0][lane]) + sh[2][0][lane]) + sh[3][0][lane];
            dbeta[c] = ((sh[0][1][lane] + sh[1][1][lane]) + sh[2][1][lane]) + sh[3][1][lane];
        }
        return;
    }
    const long n = (long)blockIdx.x * 4 + w;
    const bool act = n < Nv;
    const Drop drop(state, dxd ? p : 0.f, site);
    const float invC = 1.f / (float)C;
    for (int b = 0; act && b < Bv; ++b) {   // (Bv <= 64: checked by the entry point)
        const long m = (long)b * Nv + n;
        const float mu = mean_i[m], rs = rstd_i[m];
        float s1 = 0.f, s2 = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float g = dy[m * C + c] * gamma[c];
            s1 += g;
            s2 += g * ((xs[m * C + c] - mu) * rs);
        }
        s1 = wave_allsum(s1);
        s2 = wave_allsum(s2);
        if (lane == 0) {
            sh[w][0][b] = s1 * invC;
            sh[w][1][b] = s2 * invC;
        }
    }
    __syncthreads();
    for (int c = lane; act && c < C; c += 64) {
        float acc = 0.f;
        const float gm = gamma[c];
        for (int b = 0; b < Bv; ++b) {
            const long m = (long)b * Nv + n;
            const float mu = mean_i[m], rs = rstd_i[m];
            const float xh = (xs[m * C + c] - mu) * rs;
            float v = rs * (dy[m * C + c] * gm - sh[w][0][b] - xh * sh[w][1][b]);
            if (dres1) v += dres1[m * C + c];
            if (dres2) v += dres2[m * C + c];
            dx[m * C + c] = v;
            if (dxd) dxd[m * C + c] = v * drop((unsigned long long)(m * C + c));
            acc += v;
        }
        if (dpos) dpos[n * C + c] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ token linear
// D[i, j] = sum_k A[i sAi + k sAk] B[k sBk + j sBj]; one wave per 16 x 16 tile, four tiles along j per block.
//   forward        A = x [M, C] (C, 1), B = W [O, C] read as [k = c][j = o] (1, C): y = (x W^T + bias) drop + res
//   input gradient A = g [M, O] (O, 1), B = W (C, 1):                               dx = g W
//   weight grad.   A = g read as [i = o][k = m] (1, O), B = x (C, 1):               dW = g^T x, rowsum: dbias = sum_m g
__global__ void __launch_bounds__(256) k_gemm(const float *__restrict__ A, long sAi, long sAk, const float *__restrict__ B,
                                              long sBk, long sBj, float *__restrict__ D, long I, int J, int K,
                                              const float *__restrict__ bias, const float *__restrict__ res,
                                              float *__restrict__ rowsum, const long long *__restrict__ state, float p,
                                              int site) {
    const int lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
    const int j0 = ((int)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const long i0 = (long)blockIdx.y * 16;
    if (j0 >= J) return;
    const bool iok = i0 + r < I, jok = j0 + r < J;
    const float *ap = A + (i0 + r) * sAi, *bp = B + (long)(j0 + r) * sBj;
    float sa = 0.f;
    const f32x4a acc = mma_tile(
        K,
        [&](int, int k) {
            const float a = (iok && k < K) ? ap[k * sAk] : 0.f;
            sa += a;
            return a;
        },
        [&](int k, int) { return (jok && k < K) ? bp[k * sBk] : 0.f; });
    if (rowsum && j0 == 0) {   // sum_k A[i, k]: the four k phases of a row, added in a fixed order
        sa += __shfl_xor(sa, 16, 64);
        sa += __shfl_xor(sa, 32, 64);
        if (lane < 16 && iok) rowsum[i0 + r] = sa;
    }
    if (!jok) return;
    const Drop drop(state, p, site);
    const int j = j0 + r;
    const float bj = bias ? bias[j] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long i = i0 + 4 * kq + q;
        if (i >= I) continue;
        float v = acc[q] + bj;
        if (p > 0.f) v *= drop((unsigned long long)(i * J + j));
        if (res) v += res[i * J + j];
        D[i * J + j] = v;
    }
}

// ------------------------------------------------------------------------------------------------ attention
struct AttnGeom {
    int B, N, H, dh, C3, C;   // C = H dh, C3 = 3 C
    float scale;              // dh^-1/2
};

// S[i][j] = scale q_i . k_j for the block's 16 query rows (i0 ..) and all keys, 0 for j >= N; wave w takes key tiles w, w + 4, ..
__device__ __forceinline__ void attn_scores(float (*S)[AT_PITCH], const float *qrow0, long qstride, int nq,
                                            const float *krow0, long kstride, int nk, int NP, int dh, float scale) {
    const int lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4, w = threadIdx.x >> 6;
    for (int j0 = w * 16; j0 < NP; j0 += 64) {
        const f32x4a acc = mma_tile(
            dh, [&](int i, int k) { return (i < nq && k < dh) ? qrow0[i * qstride + k] : 0.f; },
            [&](int k, int j) { return (j0 + j < nk && k < dh) ? krow0[(j0 + j) * kstride + k] : 0.f; });
#pragma unroll
        for (int q = 0; q < 4; ++q) S[4 * kq + q][j0 + r] = acc[q] * scale;
    }
}

// out[i][d] = sum_k S[i][k] b[k][d] for d < dh (tiles of 16 over the waves), stored through `store(i, d, value)`
template <class ST>
__device__ __forceinline__ void attn_apply(const float (*S)[AT_PITCH], const float *brow0, long bstride, int nb, int NP, int dh,
                                           ST store) {
    const int lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4, w = threadIdx.x >> 6;
    for (int d0 = w * 16; d0 < dh; d0 += 64) {
        const f32x4a acc = mma_tile(
            NP, [&](int i, int k) { return S[i][k]; },
            [&](int k, int d) { return (k < nb && d0 + d < dh) ? brow0[k * bstride + d0 + d] : 0.f; });
        if (d0 + r < dh) {
#pragma unroll
            for (int q = 0; q < 4; ++q) store(4 * kq + q, d0 + r, acc[q]);
        }
    }
}

__global__ void __launch_bounds__(256) k_attn_fwd(const float *qbuf, const float *kvbuf, const float *__restrict__ res,
                                                  float *__restrict__ out, float *__restrict__ rowmax,
                                                  float *__restrict__ rowsum, AttnGeom g,
                                                  const long long *__restrict__ state, float p, int site) {
    __shared__ float S[AT_TQ][AT_PITCH];
    const int bh = blockIdx.y, b = bh / g.H, h = bh % g.H, i0 = blockIdx.x * AT_TQ;
    const int N = g.N, NP = (N + 15) & ~15, nq = min((int)AT_TQ, N - i0);
    const float *q0 = qbuf + ((long)b * N + i0) * g.C3 + h * g.dh;
    const float *k0 = kvbuf + (long)b * N * g.C3 + g.C + h * g.dh;
    attn_scores(S, q0, g.C3, nq, k0, g.C3, N, NP, g.dh, g.scale);
    __syncthreads();
    {
        const Drop drop(state, p, site);
        const int i = threadIdx.x >> 4, sub = threadIdx.x & 15;   // 16 threads per row
        if (i < nq) {
            float mx = -INFINITY;
            for (int j = sub; j < N; j += 16) mx = fmaxf(mx, S[i][j]);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            float sum = 0.f;
            for (int j = sub; j < N; j += 16) {
                const float e = expf(S[i][j] - mx);
                S[i][j] = e;
                sum += e;
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            const unsigned long long e0 = ((unsigned long long)bh * N + (i0 + i)) * N;
            for (int j = sub; j < N; j += 16) S[i][j] = (S[i][j] / sum) * drop(e0 + j);
            if (sub == 0) {
                rowmax[(long)bh * N + i0 + i] = mx;
                rowsum[(long)bh * N + i0 + i] = sum;
            }
        } else {
            for (int j = sub; j < N; j += 16) S[i][j] = 0.f;
        }
    }
    __syncthreads();
    const float *v0 = kvbuf + (long)b * N * g.C3 + 2 * g.C + h * g.dh;
    attn_apply(S, v0, g.C3, N, NP, g.dh, [&](int i, int d, float v) {
        if (i < nq) {
            const long o = ((long)b * N + i0 + i) * g.C + h * g.dh + d;
            out[o] = res ? v + res[o] : v;
        }
    });
}

// dq of the block's 16 query rows, and delta_i = sum_j P~_ij dP~_ij for k_attn_bwd_kv
__global__ void __launch_bounds__(256) k_attn_bwd_q(const float *qbuf, const float *kvbuf, const float *__restrict__ dout,
                                                    const float *__restrict__ rowmax, const float *__restrict__ rowsum,
                                                    float *__restrict__ delta, float *dqbuf, AttnGeom g,
                                                    const long long *__restrict__ state, float p, int site) {
    __shared__ float S[AT_TQ][AT_PITCH];
    __shared__ float G[AT_TQ][AT_PITCH];
    const int bh = blockIdx.y, b = bh / g.H, h = bh % g.H, i0 = blockIdx.x * AT_TQ;
    const int N = g.N, NP = (N + 15) & ~15, nq = min((int)AT_TQ, N - i0);
    const float *q0 = qbuf + ((long)b * N + i0) * g.C3 + h * g.dh;
    const float *k0 = kvbuf + (long)b * N * g.C3 + g.C + h * g.dh;
    const float *v0 = kvbuf + (long)b * N * g.C3 + 2 * g.C + h * g.dh;
    const float *do0 = dout + ((long)b * N + i0) * g.C + h * g.dh;
    attn_scores(S, q0, g.C3, nq, k0, g.C3, N, NP, g.dh, g.scale);
    attn_scores(G, do0, g.C, nq, v0, g.C3, N, NP, g.dh, 1.f);   // dP~ = dO v^T
    __syncthreads();
    {
        const Drop drop(state, p, site);
        const int i = threadIdx.x >> 4, sub = threadIdx.x & 15;
        if (i < nq) {
            const float mx = rowmax[(long)bh * N + i0 + i], inv = 1.f / rowsum[(long)bh * N + i0 + i];
            const unsigned long long e0 = ((unsigned long long)bh * N + (i0 + i)) * N;
            float dl = 0.f;
            for (int j = sub; j < N; j += 16) {
                const float pij = expf(S[i][j] - mx) * inv;
                const float dp = G[i][j] * drop(e0 + j);   // dP = dP~ mask / (1 - p)
                S[i][j] = pij;
                G[i][j] = dp;
                dl += pij * dp;
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) dl += __shfl_xor(dl, o, 64);
            for (int j = sub; j < N; j += 16) S[i][j] = S[i][j] * (G[i][j] - dl) * g.scale;
            if (sub == 0) delta[(long)bh * N + i0 + i] = dl;
        } else {
            for (int j = sub; j < N; j += 16) S[i][j] = 0.f;
        }
    }
    __syncthreads();
    attn_apply(S, k0, g.C3, N, NP, g.dh, [&](int i, int d, float v) {
        if (i < nq) dqbuf[((long)b * N + i0 + i) * g.C3 + h * g.dh + d] = v;
    });
}

// dk and dv of the block's 16 key rows: the transposed tiles St[jj][i] = scale k_j . q_i and Gt[jj][i] = v_j . dO_i
__global__ void __launch_bounds__(256) k_attn_bwd_kv(const float *qbuf, const float *kvbuf, const float *__restrict__ dout,
                                                     const float *__restrict__ rowmax, const float *__restrict__ rowsum,
                                                     const float *__restrict__ delta, float *dkvbuf, AttnGeom g,
                                                     const long long *__restrict__ state, float p, int site) {
    __shared__ float S[AT_TQ][AT_PITCH];
    __shared__ float G[AT_TQ][AT_PITCH];
    const int bh = blockIdx.y, b = bh / g.H, h = bh % g.H, j0 = blockIdx.x * AT_TQ;
    const int N = g.N, NP = (N + 15) & ~15, nk = min((int)AT_TQ, N - j0);
    const float *q0 = qbuf + (long)b * N * g.C3 + h * g.dh;
    const float *k0 = kvbuf + ((long)b * N + j0) * g.C3 + g.C + h * g.dh;
    const float *v0 = kvbuf + ((long)b * N + j0) * g.C3 + 2 * g.C + h * g.dh;
    const float *do0 = dout + (long)b * N * g.C + h * g.dh;
    attn_scores(S, k0, g.C3, nk, q0, g.C3, N, NP, g.dh, g.scale);
    attn_scores(G, v0, g.C3, nk, do0, g.C, N, NP, g.dh, 1.f);
    __syncthreads();
    {
        const Drop drop(state, p, site);
        for (int idx = threadIdx.x; idx < AT_TQ * NP; idx += 256) {
            const int jj = idx / NP, i = idx - jj * NP;
            float ds = 0.f, pt = 0.f;
            if (jj < nk && i < N) {
                const long row = (long)bh * N + i;
                const float pij = expf(S[jj][i] - rowmax[row]) / rowsum[row];
                const float m = drop(((unsigned long long)row) * N + (j0 + jj));
                pt = pij * m;
                ds = pij * (G[jj][i] * m - delta[row]) * g.scale;
            }
            S[jj][i] = ds;
            G[jj][i] = pt;
        }
    }
    __syncthreads();
    float *dk0 = dkvbuf + ((long)b * N + j0) * g.C3 + g.C + h * g.dh;
    attn_apply(S, q0, g.C3, N, NP, g.dh, [&](int jj, int d, float v) {
        if (jj < nk) dk0[(long)jj * g.C3 + d] = v;
    });
    attn_apply(G, do0, g.C, N, NP, g.dh, [&](int jj, int d, float v) {
        if (jj < nk) dk0[(long)jj * g.C3 + g.C + d] = v;
    });
}

static int attn_geom(AttnGeom &g, int B, int N, int H, int dh, const char *what) {
    MVD_REQUIRE(B > 0 && N > 0 && H > 0, "%s: bad shape", what);
    MVD_REQUIRE(N <= AT_NMAX, "%s: %d tokens, the kernel holds a row of at most %d scores in LDS", what, N, (int)AT_NMAX);
    MVD_REQUIRE(dh >= 4 && dh <= 64 && dh % 4 == 0, "%s: head dimension %d (4..64, multiple of 4)", what, dh);
    MVD_REQUIRE((long)B * H <= 65535, "%s: batch x heads above the grid limit", what);
    g.B = B; g.N = N; g.H = H; g.dh = dh; g.C = H * dh; g.C3 = 3 * g.C;
    g.scale = (float)(1.0 / sqrt((double)dh));
    return 0;
}

}  // namespace mvd

using namespace mvd;

extern "C" {

int mvd_dropout_tick(long long *state, void *stream) {
    MVD_REQUIRE(state && (((uintptr_t)state) & 7) == 0, "dropout_tick: bad arguments");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_dropout_tick, dim3(1), dim3(1), 0, s, state);
    return check_launch("dropout_tick");
}

int mvd_dropout_mask(unsigned long long seed, unsigned long long t, int site, float p, long n, unsigned char *out,
                     void *stream) {
    MVD_REQUIRE(out && n > 0 && site >= 0 && p >= 0.f && p < 1.f, "dropout_mask: bad arguments");
    hipStream_t s = as_stream(stream);
    long bx = cdiv(n, 256);
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(k_dropout_mask, dim3(bx), dim3(256), 0, s, seed, t, site, p, n, out);
    return check_launch("dropout_mask");
}

int mvd_layernorm_fwd(const float *x, const float *pos, float *xs, float *y, float *mean, float *rstd, const float *gamma,
                      const float *beta, long M, int C, long Npos, float eps, void *stream) {
    MVD_REQUIRE(x && y && mean && rstd && gamma && beta && M > 0 && C > 0, "layernorm_fwd: bad arguments");
    MVD_REQUIRE(!pos || (Npos > 0 && M % Npos == 0), "layernorm_fwd: %ld rows are no whole number of %ld positions", M, Npos);
    MVD_REQUIRE(cdiv(M, 4) <= 0x7fffffffL, "layernorm_fwd: too many rows");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_layernorm_fwd, dim3(cdiv(M, 4)), dim3(256), 0, s, x, pos, xs, y, mean, rstd, gamma, beta, M, C, Npos,
                       eps);
    return check_launch("layernorm_fwd");
}

int mvd_layernorm_bwd(const float *dy, const float *xs, const float *mean, const float *rstd, const float *gamma,
                      const float *dres1, const float *dres2, float *dx, float *dxd, float *dgamma, float *dbeta,
                      float *dpos, long M, int C, long Npos, const long long *state, float p, int site, void *stream) {
    MVD_REQUIRE(dy && xs && mean && rstd && gamma && dx && dgamma && dbeta && M > 0 && C > 0, "layernorm_bwd: bad arguments");
    MVD_REQUIRE(!dpos || (Npos > 0 && M % Npos == 0), "layernorm_bwd: %ld rows are no whole number of %ld positions", M, Npos);
    MVD_REQUIRE(!dxd || p == 0.f || (state && p > 0.f && p < 1.f), "layernorm_bwd: dropout needs the device state and 0 <= p < 1");
    const long Nv = dpos ? Npos : M;
    const long Bv = M / Nv;
    MVD_REQUIRE(Bv <= 64, "layernorm_bwd: batch %ld above 64 with a position embedding", Bv);
    const long nrow = cdiv(Nv, 4);
    MVD_REQUIRE(nrow + cdiv(C, 64) <= 0x7fffffffL, "layernorm_bwd: too many rows");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_layernorm_bwd, dim3(nrow + cdiv(C, 64)), dim3(256), 0, s, dy, xs, mean, rstd, gamma, dres1, dres2, dx,
                       dxd, dgamma, dbeta, dpos, (int)Bv, Nv, C, (int)nrow, state, p, site);
    return check_launch("layernorm_bwd");
}

int mvd_linear_fwd(const float *x, const float *w, const float *bias, const float *res, float *y, long M, int C, int O,
                   const long long *state, float p, int site, void *stream) {
    MVD_REQUIRE(x && w && y && M > 0 && C > 0 && O > 0, "linear_fwd: bad arguments");
    MVD_REQUIRE(C % 8 == 0 && O % 8 == 0, "linear_fwd: C = %d and O = %d must be multiples of 8", C, O);
    MVD_REQUIRE(p == 0.f || (state && p > 0.f && p < 1.f), "linear_fwd: dropout needs the device state and 0 <= p < 1");
    MVD_REQUIRE(cdiv(M, 16) <= 65535, "linear_fwd: too many rows");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_gemm, dim3(cdiv(cdiv(O, 16), 4), cdiv(M, 16)), dim3(256), 0, s, x, (long)C, 1L, w, 1L, (long)C, y, M, O,
                       C, bias, res, (float *)nullptr, state, p, site);
    return check_launch("linear_fwd");
}

int mvd_linear_bwd(const float *g, const float *x, const float *w, float *dx, float *dw, float *db, long M, int C, int O,
                   void *stream) {
    MVD_REQUIRE(g && x && w && M > 0 && C > 0 && O > 0, "linear_bwd: bad arguments");
    MVD_REQUIRE(C % 8 == 0 && O % 8 == 0, "linear_bwd: C = %d and O = %d must be multiples of 8", C, O);
    MVD_REQUIRE(cdiv(M, 16) <= 65535 && M <= 0x7fffffffL, "linear_bwd: too many rows");
    MVD_REQUIRE(!db || dw, "linear_bwd: the bias gradient rides in the weight-gradient launch");
    hipStream_t s = as_stream(stream);
    const long long *nostate = nullptr;
    if (dx) {
        hipLaunchKernelGGL(k_gemm, dim3(cdiv(cdiv(C, 16), 4), cdiv(M, 16)), dim3(256), 0, s, g, (long)O, 1L, w, (long)C, 1L, dx,
                           M, C, O, (const float *)nullptr, (const float *)nullptr, (float *)nullptr, nostate, 0.f, 0);
        if (check_launch("linear_bwd (input gradient)")) return 1;
    }
    if (dw) {
        hipLaunchKernelGGL(k_gemm, dim3(cdiv(cdiv(C, 16), 4), cdiv(O, 16)), dim3(256), 0, s, g, 1L, (long)O, x, (long)C, 1L, dw,
                           (long)O, C, (int)M, (const float *)nullptr, (const float *)nullptr, db, nostate, 0.f, 0);
        if (check_launch("linear_bwd (weight gradient)")) return 1;
    }
    return 0;
}

int mvd_attention_fwd(const float *qbuf, const float *kvbuf, const float *res, float *out, float *rowmax, float *rowsum, int B,
                      int N, int H, int dh, const long long *state, float p, int site, void *stream) {
    MVD_REQUIRE(qbuf && kvbuf && out && rowmax && rowsum, "attention_fwd: bad arguments");
    MVD_REQUIRE(p == 0.f || (state && p > 0.f && p < 1.f), "attention_fwd: dropout needs the device state and 0 <= p < 1");
    AttnGeom g;
    if (int rc = attn_geom(g, B, N, H, dh, "attention_fwd")) return rc;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_attn_fwd, dim3(cdiv(N, AT_TQ), B * H), dim3(256), 0, s, qbuf, kvbuf, res, out, rowmax, rowsum, g, state,
                       p, site);
    return check_launch("attention_fwd");
}

int mvd_attention_bwd(const float *qbuf, const float *kvbuf, const float *dout, const float *rowmax, const float *rowsum,
                      float *delta, float *dqbuf, float *dkvbuf, int B, int N, int H, int dh, const long long *state, float p,
                      int site, void *stream) {
    MVD_REQUIRE(qbuf && kvbuf && dout && rowmax && rowsum && delta && dqbuf && dkvbuf, "attention_bwd: bad arguments");
    MVD_REQUIRE(p == 0.f || (state && p > 0.f && p < 1.f), "attention_bwd: dropout needs the device state and 0 <= p < 1");
    AttnGeom g;
    if (int rc = attn_geom(g, B, N, H, dh, "attention_bwd")) return rc;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_attn_bwd_q, dim3(cdiv(N, AT_TQ), B * H), dim3(256), 0, s, qbuf, kvbuf, dout, rowmax, rowsum, delta, dqbuf,
                       g, state, p, site);
    if (check_launch("attention_bwd (dq)")) return 1;
    hipLaunchKernelGGL(k_attn_bwd_kv, dim3(cdiv(N, AT_TQ), B * H), dim3(256), 0, s, qbuf, kvbuf, dout, rowmax, rowsum, delta,
                       dkvbuf, g, state, p, site);
    return check_launch("attention_bwd (dk, dv)");
}
}
