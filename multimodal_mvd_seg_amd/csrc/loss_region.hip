// Region-based training and the ignore label: fused sigmoid + BCE + soft-Dice over R overlapping regions
// (DC_and_BCE_loss), the ignore-label form of the softmax DC+CE loss, and their online-evaluation counts.
// Same structure as k_dcce_* (loss.hip): one pass over the planar logits with all heads of a voxel in flight, fp64
// per-thread partials -> fixed-order block tree -> partials -> fixed-order second stage.  No float atomics.
//
// Targets of the region kernels come in two forms (template flag PLANES):
//   label map  float [N][V]: label -> bitmask through a 256-entry table staged in LDS (bit r: the label belongs to region
//              r, bit 31: the label is the ignore label; the mvd_seg_label_mask convention).  Labels are truncated like
//              .long() and clamped to 0..255.
//   planes     float [N][TP][V], TP = R (+1: the ignore plane, last), the output of ConvertSegmentationToRegionsTransform;
//              a plane value >= 0.5 is a set bit.
// Both forms are reduced to the same per-voxel bitmask first, so they give bit-identical results.
#include "common.h"

namespace mvd {

constexpr int RKMAX = 8;              // heads (the KMAX of loss.hip)
constexpr int RNV = 3 * RKMAX + 2;    // I, P, G per head + loss sum + valid voxels
constexpr unsigned IGNORE_BIT = 0x80000000u;

struct LabelLut {
    uint32_t m[256];
};

__device__ __forceinline__ int label_index(float t) {
    const int y = (int)t;  // .long() truncation
    return y < 0 ? 0 : (y > 255 ? 255 : y);
}

// bitmask of voxel v (see the head of the file); R, TP uniform
template <bool PLANES>
__device__ __forceinline__ unsigned voxel_bits(const float *__restrict__ tn, const uint32_t *lut, long V, long v, int R,
                                               int TP) {
    if (!PLANES) return lut[label_index(tn[v])];
    float y[RKMAX + 1];
#pragma unroll
    for (int r = 0; r < RKMAX + 1; r++) y[r] = tn[(size_t)(r < TP ? r : TP - 1) * V + v];  // all planes in flight
    unsigned b = 0;
#pragma unroll
    for (int r = 0; r < RKMAX; r++)
        if (r < R && y[r] >= 0.5f) b |= 1u << r;
#pragma unroll
    for (int r = 1; r < RKMAX + 1; r++)
        if (r == R && TP > R && y[r] >= 0.5f) b |= IGNORE_BIT;
    return b;
}

// sigma(z) and softplus(-|z|) = log1p(exp(-|z|)) from one exponential
__device__ __forceinline__ void sigmoid_sp(float z, float &sg, float &sp) {
    const float e = expf(-fabsf(z));
    const float inv = 1.0f / (1.0f + e);
    sg = z >= 0.f ? inv : e * inv;
    sp = log1pf(e);
}

template <bool PLANES>
__global__ __launch_bounds__(256) void k_dcbce_fwd(const float *__restrict__ logits, const float *__restrict__ target,
                                                   LabelLut lutv, double *__restrict__ partial, int N, long V, int R,
                                                   int TP) {
    __shared__ double red[RNV * 16];
    __shared__ uint32_t lut[256];
    if (!PLANES) {
        lut[threadIdx.x] = lutv.m[threadIdx.x];  // blockDim.x == 256
        __syncthreads();
    }
    const int n = blockIdx.y;
    const float *ln = logits + (size_t)n * R * V;
    const float *tn = target + (size_t)n * (PLANES ? TP : 1) * V;
    double acc[RNV];
#pragma unroll
    for (int i = 0; i < RNV; i++) acc[i] = 0.0;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        float z[RKMAX];
#pragma unroll
        for (int r = 0; r < RKMAX; r++) z[r] = ln[(size_t)(r < R ? r : R - 1) * V + v];  // all heads in flight (no predicate)
        const unsigned bits = voxel_bits<PLANES>(tn, lut, V, v, R, TP);
        const float m = (bits & IGNORE_BIT) ? 0.f : 1.f;
        float bce = 0.f;
#pragma unroll
        for (int r = 0; r < RKMAX; r++)
            if (r < R) {
                const float y = (float)((bits >> r) & 1u);
                float sg, sp;
                sigmoid_sp(z[r], sg, sp);
                bce += fmaxf(z[r], 0.f) - z[r] * y + sp;
                const float ms = m * sg;
                acc[3 * r + 0] += (double)(ms * y);
                acc[3 * r + 1] += (double)ms;
                acc[3 * r + 2] += (double)(m * y);
            }
        acc[3 * RKMAX] += (double)(m * bce);
        acc[3 * RKMAX + 1] += (double)m;
    }
    block_sum<RNV>(acc, red);
    if (threadIdx.x == 0) {
        double *po = partial + ((size_t)blockIdx.x * N + n) * (3 * R + 2);
#pragma unroll
        for (int r = 0; r < RKMAX; r++)  // static indices: a run-time-indexed acc[] would live in scratch (loss.hip)
            if (r < R) {
                po[3 * r + 0] = acc[3 * r + 0];
                po[3 * r + 1] = acc[3 * r + 1];
                po[3 * r + 2] = acc[3 * r + 2];
            }
        po[3 * R] = acc[3 * RKMAX];
        po[3 * R + 1] = acc[3 * RKMAX + 1];
    }
}

// Scalar composition for stats [N][3K+2].  mode 0: loss sum / (N*K*V) (BCE, no ignore label); 1: loss sum /
// clip(valid voxels, 1e-8) (BCE with the ignore label: voxels, not voxels x heads, as upstream); 2: loss sum / valid
// voxels, 0 when there is none (CE with ignore_index).  loss[3] = the factor c the backward multiplies (p - y) with.
// The Dice part is the arithmetic of k_dcce_finalize.
__global__ void k_masked_finalize(const float *__restrict__ stats, int N, const float *__restrict__ dstats, int Nd,
                                  float *__restrict__ loss, float *__restrict__ coef, long V, int K, int batch_dice,
                                  int do_bg, float smooth, float w_ce, float w_dice, int mode) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int S = 3 * K + 2;
    double ce = 0, cnt = 0;
    for (int n = 0; n < N; n++) {
        ce += (double)stats[(size_t)n * S + 3 * K];
        cnt += (double)stats[(size_t)n * S + 3 * K + 1];
    }
    double c;
    if (mode == 0)
        c = 1.0 / ((double)N * (double)K * (double)V);
    else if (mode == 1)
        c = 1.0 / (cnt < 1e-8 ? 1e-8 : cnt);
    else
        c = cnt > 0.0 ? 1.0 / cnt : 0.0;
    ce *= c;
    const int k0 = do_bg ? 0 : 1;
    double dcsum = 0;
    for (size_t i = 0; i < (size_t)Nd * K * 2; i++) coef[i] = 0.f;
    if (K - k0 > 0) {
        if (batch_dice) {
            const double nk = (double)(K - k0);
            for (int k = k0; k < K; k++) {
                float I = 0, P = 0, G = 0;  // torch sums the per-sample fp32 values in fp32
                for (int n = 0; n < Nd; n++) {
                    I += dstats[(size_t)n * S + 3 * k + 0];
                    P += dstats[(size_t)n * S + 3 * k + 1];
                    G += dstats[(size_t)n * S + 3 * k + 2];
                }
                float den = G + P + smooth;
                const bool clipped = den < 1e-8f;
                if (clipped) den = 1e-8f;
                const float num = 2.f * I + smooth;
                dcsum += (double)(num / den);
                const float cI = (float)(-(1.0 / nk) * 2.0 / (double)den);
                const float cP = clipped ? 0.f : (float)((1.0 / nk) * (double)num / ((double)den * (double)den));
                for (int n = 0; n < Nd; n++) {
                    coef[((size_t)n * K + k) * 2 + 0] = w_dice * cI;
                    coef[((size_t)n * K + k) * 2 + 1] = w_dice * cP;
                }
            }
            dcsum /= nk;
        } else {
            const double nk = (double)Nd * (double)(K - k0);
            for (int n = 0; n < Nd; n++)
                for (int k = k0; k < K; k++) {
                    const float I = dstats[(size_t)n * S + 3 * k + 0], P = dstats[(size_t)n * S + 3 * k + 1],
                                G = dstats[(size_t)n * S + 3 * k + 2];
                    float den = G + P + smooth;
                    const bool clipped = den < 1e-8f;
                    if (clipped) den = 1e-8f;
                    const float num = 2.f * I + smooth;
                    dcsum += (double)(num / den);
                    coef[((size_t)n * K + k) * 2 + 0] = w_dice * (float)(-(1.0 / nk) * 2.0 / (double)den);
                    coef[((size_t)n * K + k) * 2 + 1] =
                        clipped ? 0.f : w_dice * (float)((1.0 / nk) * (double)num / ((double)den * (double)den));
                }
            dcsum /= nk;
        }
    }
    loss[1] = (float)ce;
    loss[2] = (float)(-dcsum);
    loss[0] = w_ce * (float)ce + w_dice * (float)(-dcsum);
    loss[3] = (float)c;
}

template <bool PLANES>
__global__ __launch_bounds__(256) void k_dcbce_bwd(const float *__restrict__ logits, const float *__restrict__ target,
                                                   LabelLut lutv, const float *__restrict__ coef,
                                                   const float *__restrict__ loss, const float *__restrict__ gscale_dev,
                                                   float gscale_host, float *__restrict__ dlogits, long V, int R, int TP,
                                                   float w_ce) {
    __shared__ uint32_t lut[256];
    if (!PLANES) {
        lut[threadIdx.x] = lutv.m[threadIdx.x];
        __syncthreads();
    }
    const int n = blockIdx.y;
    const float *ln = logits + (size_t)n * R * V;
    const float *tn = target + (size_t)n * (PLANES ? TP : 1) * V;
    float *dn = dlogits + (size_t)n * R * V;
    const float g = gscale_host * (gscale_dev ? gscale_dev[0] : 1.0f);
    const float cew = w_ce * loss[3];
    float cI[RKMAX], cP[RKMAX];
#pragma unroll
    for (int r = 0; r < RKMAX; r++)
        if (r < R) {
            cI[r] = coef[((size_t)n * R + r) * 2 + 0];
            cP[r] = coef[((size_t)n * R + r) * 2 + 1];
        }
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        float z[RKMAX];
#pragma unroll
        for (int r = 0; r < RKMAX; r++) z[r] = ln[(size_t)(r < R ? r : R - 1) * V + v];
        const unsigned bits = voxel_bits<PLANES>(tn, lut, V, v, R, TP);
        const bool valid = !(bits & IGNORE_BIT);
#pragma unroll
        for (int r = 0; r < RKMAX; r++)
            if (r < R) {
                const bool y = (bits >> r) & 1u;
                const float e = expf(-fabsf(z[r]));
                const float inv = 1.0f / (1.0f + e);
                const float sg = z[r] >= 0.f ? inv : e * inv;
                const float d = cew * (sg - (y ? 1.f : 0.f)) + sg * (1.f - sg) * (cP[r] + (y ? cI[r] : 0.f));
                dn[(size_t)r * V + v] = valid ? g * d : 0.f;  // (a select, not a product: an ignored voxel is an exact 0)
            }
    }
}

// ------------------------------------------------------------------------------------------- softmax DC+CE, ignore label
__global__ __launch_bounds__(256) void k_dcce_masked_fwd(const float *__restrict__ logits, const float *__restrict__ target,
                                                         double *__restrict__ partial, int N, long V, int K, int ignore) {
    __shared__ double red[RNV * 16];
    const int n = blockIdx.y;
    const float *ln = logits + (size_t)n * K * V;
    const float *tn = target + (size_t)n * V;
    double acc[RNV];
#pragma unroll
    for (int i = 0; i < RNV; i++) acc[i] = 0.0;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        float z[RKMAX];
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < RKMAX; k++) z[k] = ln[(size_t)(k < K ? k : K - 1) * V + v];
#pragma unroll
        for (int k = 0; k < RKMAX; k++)
            if (k < K) mx = fmaxf(mx, z[k]);
        const int yi = (int)tn[v];
        const bool valid = yi != ignore;
        const int y = yi < 0 ? 0 : (yi >= K ? K - 1 : yi);  // (an ignored voxel contributes nothing below)
        float s = 0.f, zy = 0.f;
#pragma unroll
        for (int k = 0; k < RKMAX; k++)
            if (k < K) {
                const float d = z[k] - mx;
                if (k == y) zy = d;
                z[k] = expf(d);
                s += z[k];
            }
        if (valid) {
            const float inv = 1.0f / s;
            acc[3 * RKMAX] += (double)(logf(s) - zy);
            acc[3 * RKMAX + 1] += 1.0;
#pragma unroll
            for (int k = 0; k < RKMAX; k++)
                if (k < K) {
                    const float p = z[k] * inv;
                    if (k == y) {
                        acc[3 * k + 0] += (double)p;
                        acc[3 * k + 2] += 1.0;
                    }
                    acc[3 * k + 1] += (double)p;
                }
        }
    }
    block_sum<RNV>(acc, red);
    if (threadIdx.x == 0) {
        double *po = partial + ((size_t)blockIdx.x * N + n) * (3 * K + 2);
#pragma unroll
        for (int k = 0; k < RKMAX; k++)
            if (k < K) {
                po[3 * k + 0] = acc[3 * k + 0];
                po[3 * k + 1] = acc[3 * k + 1];
                po[3 * k + 2] = acc[3 * k + 2];
            }
        po[3 * K] = acc[3 * RKMAX];
        po[3 * K + 1] = acc[3 * RKMAX + 1];
    }
}

__global__ __launch_bounds__(256) void k_dcce_masked_bwd(const float *__restrict__ logits, const float *__restrict__ target,
                                                         const float *__restrict__ coef, const float *__restrict__ loss,
                                                         const float *__restrict__ gscale_dev, float gscale_host,
                                                         float *__restrict__ dlogits, long V, int K, float w_ce,
                                                         int ignore) {
    const int n = blockIdx.y;
    const float *ln = logits + (size_t)n * K * V;
    const float *tn = target + (size_t)n * V;
    float *dn = dlogits + (size_t)n * K * V;
    const float g = gscale_host * (gscale_dev ? gscale_dev[0] : 1.0f);
    const float cew = w_ce * loss[3];
    float cI[RKMAX], cP[RKMAX];
#pragma unroll
    for (int k = 0; k < RKMAX; k++)
        if (k < K) {
            cI[k] = coef[((size_t)n * K + k) * 2 + 0];
            cP[k] = coef[((size_t)n * K + k) * 2 + 1];
        }
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        float z[RKMAX];
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < RKMAX; k++) z[k] = ln[(size_t)(k < K ? k : K - 1) * V + v];
#pragma unroll
        for (int k = 0; k < RKMAX; k++)
            if (k < K) mx = fmaxf(mx, z[k]);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < RKMAX; k++)
            if (k < K) {
                z[k] = expf(z[k] - mx);
                s += z[k];
            }
        const float inv = 1.0f / s;
        const int yi = (int)tn[v];
        const bool valid = yi != ignore;
        const int y = yi < 0 ? 0 : (yi >= K ? K - 1 : yi);
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < RKMAX; k++)
            if (k < K) {
                z[k] *= inv;
                const float q = cP[k] + (k == y ? cI[k] : 0.f);
                dot += z[k] * q;
            }
#pragma unroll
        for (int k = 0; k < RKMAX; k++)
            if (k < K) {
                const float q = cP[k] + (k == y ? cI[k] : 0.f);
                const float d = cew * (z[k] - (k == y ? 1.f : 0.f)) + z[k] * (q - dot);
                dn[(size_t)k * V + v] = valid ? g * d : 0.f;
            }
    }
}

// ------------------------------------------------------------------------------------------- online-evaluation counts
// Integer sums only: per-lane uint32 counters with static indices, 64-bit from the wave reduction on, one integer atomic per
// counter and wave.  A head predicts a voxel iff its logit is > 0.
template <bool PLANES>
__global__ __launch_bounds__(256) void k_sigmoid_counts(const float *__restrict__ logits, const float *__restrict__ target,
                                                        LabelLut lutv, unsigned long long *__restrict__ counts, long V,
                                                        int R, int TP) {
    __shared__ uint32_t lut[256];
    if (!PLANES) {
        lut[threadIdx.x] = lutv.m[threadIdx.x];
        __syncthreads();
    }
    const int n = blockIdx.y;
    const float *ln = logits + (size_t)n * R * V;
    const float *tn = target + (size_t)n * (PLANES ? TP : 1) * V;
    unsigned c[3 * RKMAX];
#pragma unroll
    for (int i = 0; i < 3 * RKMAX; i++) c[i] = 0;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        float z[RKMAX];
#pragma unroll
        for (int r = 0; r < RKMAX; r++) z[r] = ln[(size_t)(r < R ? r : R - 1) * V + v];
        const unsigned bits = voxel_bits<PLANES>(tn, lut, V, v, R, TP);
        const unsigned m = (bits & IGNORE_BIT) ? 0u : 1u;
#pragma unroll
        for (int r = 0; r < RKMAX; r++)
            if (r < R) {
                const unsigned p = z[r] > 0.f ? 1u : 0u, y = (bits >> r) & 1u;
                c[3 * r + 0] += m & p & y;
                c[3 * r + 1] += m & p & (y ^ 1u);
                c[3 * r + 2] += m & (p ^ 1u) & y;
            }
    }
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < 3 * RKMAX; i++)
        if (i < 3 * R) {
            unsigned long long s = c[i];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
            if (lane == 0 && s) atomicAdd(&counts[i], s);
        }
}

__global__ __launch_bounds__(256) void k_argmax_counts_masked(const float *__restrict__ logits,
                                                              const float *__restrict__ target,
                                                              unsigned long long *__restrict__ counts, long V, int K,
                                                              int ignore) {
    __shared__ unsigned int c_s[RKMAX * 3];
    const int n = blockIdx.y;
    if (threadIdx.x < RKMAX * 3) c_s[threadIdx.x] = 0;
    __syncthreads();
    const float *ln = logits + (size_t)n * K * V;
    const float *tn = target + (size_t)n * V;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        int best = 0;
        float bv = ln[v];
        for (int k = 1; k < K; k++) {
            const float z = ln[(size_t)k * V + v];
            if (z > bv) {  // first maximum wins (torch.argmax)
                bv = z;
                best = k;
            }
        }
        const int yi = (int)tn[v];
        if (yi == ignore) continue;
        const int y = yi < 0 ? 0 : (yi >= K ? K - 1 : yi);
        if (best == y)
            atomicAdd(&c_s[3 * y + 0], 1u);
        else {
            atomicAdd(&c_s[3 * best + 1], 1u);
            atomicAdd(&c_s[3 * y + 2], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < K * 3 && c_s[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)c_s[threadIdx.x]);
}

// planes[n][p][v] = label map -> region planes (+ the ignore plane, last)
__global__ __launch_bounds__(256) void k_seg_to_regions(const float *__restrict__ seg, LabelLut lutv, float *__restrict__ planes,
                                                        long V, int R, int TP) {
    __shared__ uint32_t lut[256];
    lut[threadIdx.x] = lutv.m[threadIdx.x];
    __syncthreads();
    const int n = blockIdx.y;
    const float *sn = seg + (size_t)n * V;
    float *pn = planes + (size_t)n * TP * V;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        const unsigned bits = lut[label_index(sn[v])];
        for (int r = 0; r < R; r++) pn[(size_t)r * V + v] = (float)((bits >> r) & 1u);
        if (TP > R) pn[(size_t)R * V + v] = (bits & IGNORE_BIT) ? 1.f : 0.f;
    }
}

}  // namespace mvd

using namespace mvd;

static inline long rgrid_for(long n, long cap) {
    long b = cdiv(n, 256);
    if (b > cap) b = cap;
    return b < 1 ? 1 : b;
}
static inline long rcap_per_n(long total_blocks, int N) {
    const long c = total_blocks / (N > 0 ? N : 1);
    return c > 0 ? c : 1;
}

// target_form 0: label map + table (host array of 256 masks), 1: R planes, 2: R planes + the ignore plane
static int region_form(const char *what, int target_form, const uint32_t *lut_host, int R, LabelLut &lut, int &TP) {
    MVD_REQUIRE(target_form >= 0 && target_form <= 2, "%s: target_form must be 0 (label map), 1 (planes) or 2 (planes + ignore)",
                what);
    memset(&lut, 0, sizeof(lut));
    TP = R + (target_form == 2 ? 1 : 0);
    if (target_form == 0) {
        MVD_REQUIRE(lut_host, "%s: the label-map form needs the label table", what);
        const uint32_t allowed = (R >= 31 ? 0x7fffffffu : ((1u << R) - 1u)) | IGNORE_BIT;
        for (int i = 0; i < 256; i++) {
            MVD_REQUIRE((lut_host[i] & ~allowed) == 0, "%s: label %d has a bit outside the %d regions", what, i, R);
            lut.m[i] = lut_host[i];
        }
    }
    return 0;
}

extern "C" {

size_t mvd_dcbce_workspace_bytes(int N, long V, int R) {
    const long bx = rgrid_for(V, rcap_per_n(2048, N));
    return (size_t)bx * N * (3 * R + 2) * sizeof(double) + 256;
}

int mvd_dcbce_fwd(const float *logits, const float *target, int target_form, const uint32_t *lut_host, float *stats, int N,
                  long V, int R, void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(logits && target && stats && ws, "dcbce_fwd: null pointer");
    MVD_REQUIRE(N > 0 && N <= 65535 && V > 0 && R >= 1 && R <= RKMAX, "dcbce_fwd: bad shape (1 <= R <= 8 heads)");
    MVD_REQUIRE(ws_bytes >= mvd_dcbce_workspace_bytes(N, V, R), "dcbce_fwd: workspace too small");
    LabelLut lut;
    int TP;
    if (int rc = region_form("dcbce_fwd", target_form, lut_host, R, lut, TP)) return rc;
    const long bx = rgrid_for(V, rcap_per_n(2048, N));
    double *partial = reinterpret_cast<double *>(ws);
    hipStream_t s = as_stream(stream);
    if (target_form == 0)
        hipLaunchKernelGGL(k_dcbce_fwd<false>, dim3(bx, N), dim3(256), 0, s, logits, target, lut, partial, N, V, R, TP);
    else
        hipLaunchKernelGGL(k_dcbce_fwd<true>, dim3(bx, N), dim3(256), 0, s, logits, target, lut, partial, N, V, R, TP);
    if (check_launch("dcbce_fwd")) return 1;
    return reduce_partials(partial, stats, (int)bx, N * (3 * R + 2), s);
}

static int masked_finalize(const char *what, const float *stats, int N, const float *dstats, int Nd, float *loss,
                           float *coef, long V, int K, int batch_dice, int do_bg, float smooth, float w_ce, float w_dice,
                           int mode, void *stream) {
    MVD_REQUIRE(stats && loss && coef && N > 0 && V > 0 && K >= 1 && K <= RKMAX, "%s: bad arguments", what);
    if (!dstats) {
        dstats = stats;
        Nd = N;
    }
    MVD_REQUIRE(Nd > 0, "%s: empty Dice sample set", what);
    hipLaunchKernelGGL(k_masked_finalize, dim3(1), dim3(64), 0, as_stream(stream), stats, N, dstats, Nd, loss, coef, V, K,
                       batch_dice, do_bg, smooth, w_ce, w_dice, mode);
    return check_launch(what);
}

int mvd_dcbce_finalize(const float *stats, int N, const float *dstats, int Nd, float *loss, float *coef, long V, int R,
                       int batch_dice, int do_bg, int use_ignore_label, float smooth, float w_ce, float w_dice,
                       void *stream) {
    return masked_finalize("dcbce_finalize", stats, N, dstats, Nd, loss, coef, V, R, batch_dice, do_bg, smooth, w_ce, w_dice,
                           use_ignore_label ? 1 : 0, stream);
}

int mvd_dcbce_bwd(const float *logits, const float *target, int target_form, const uint32_t *lut_host, const float *coef,
                  const float *loss, const float *gscale_dev, float gscale_host, float *dlogits, int N, long V, int R,
                  float w_ce, void *stream) {
    MVD_REQUIRE(logits && target && coef && loss && dlogits, "dcbce_bwd: null pointer");
    MVD_REQUIRE(N > 0 && N <= 65535 && V > 0 && R >= 1 && R <= RKMAX, "dcbce_bwd: bad shape (1 <= R <= 8 heads)");
    LabelLut lut;
    int TP;
    if (int rc = region_form("dcbce_bwd", target_form, lut_host, R, lut, TP)) return rc;
    const long bx = rgrid_for(V, rcap_per_n(4096, N));
    hipStream_t s = as_stream(stream);
    if (target_form == 0)
        hipLaunchKernelGGL(k_dcbce_bwd<false>, dim3(bx, N), dim3(256), 0, s, logits, target, lut, coef, loss, gscale_dev,
                           gscale_host, dlogits, V, R, TP, w_ce);
    else
        hipLaunchKernelGGL(k_dcbce_bwd<true>, dim3(bx, N), dim3(256), 0, s, logits, target, lut, coef, loss, gscale_dev,
                           gscale_host, dlogits, V, R, TP, w_ce);
    return check_launch("dcbce_bwd");
}

size_t mvd_dcce_masked_workspace_bytes(int N, long V, int K) { return mvd_dcbce_workspace_bytes(N, V, K); }

int mvd_dcce_masked_fwd(const float *logits, const float *target, float *stats, int N, long V, int K, int ignore_label,
                        void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(logits && target && stats && ws, "dcce_masked_fwd: null pointer");
    MVD_REQUIRE(N > 0 && N <= 65535 && V > 0 && K >= 2 && K <= RKMAX, "dcce_masked_fwd: bad shape (2<=K<=8)");
    MVD_REQUIRE(ws_bytes >= mvd_dcce_masked_workspace_bytes(N, V, K), "dcce_masked_fwd: workspace too small");
    const long bx = rgrid_for(V, rcap_per_n(2048, N));
    double *partial = reinterpret_cast<double *>(ws);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_dcce_masked_fwd, dim3(bx, N), dim3(256), 0, s, logits, target, partial, N, V, K, ignore_label);
    if (check_launch("dcce_masked_fwd")) return 1;
    return reduce_partials(partial, stats, (int)bx, N * (3 * K + 2), s);
}

int mvd_dcce_masked_finalize(const float *stats, int N, const float *dstats, int Nd, float *loss, float *coef, long V, int K,
                             int batch_dice, int do_bg, float smooth, float w_ce, float w_dice, void *stream) {
    MVD_REQUIRE(K >= 2, "dcce_masked_finalize: K >= 2");
    return masked_finalize("dcce_masked_finalize", stats, N, dstats, Nd, loss, coef, V, K, batch_dice, do_bg, smooth, w_ce,
                           w_dice, 2, stream);
}

int mvd_dcce_masked_bwd(const float *logits, const float *target, const float *coef, const float *loss,
                        const float *gscale_dev, float gscale_host, float *dlogits, int N, long V, int K, float w_ce,
                        int ignore_label, void *stream) {
    MVD_REQUIRE(logits && target && coef && loss && dlogits, "dcce_masked_bwd: null pointer");
    MVD_REQUIRE(N > 0 && N <= 65535 && V > 0 && K >= 2 && K <= RKMAX, "dcce_masked_bwd: bad shape");
    const long bx = rgrid_for(V, rcap_per_n(4096, N));
    hipLaunchKernelGGL(k_dcce_masked_bwd, dim3(bx, N), dim3(256), 0, as_stream(stream), logits, target, coef, loss,
                       gscale_dev, gscale_host, dlogits, V, K, w_ce, ignore_label);
    return check_launch("dcce_masked_bwd");
}

int mvd_sigmoid_counts(const float *logits, const float *target, int target_form, const uint32_t *lut_host,
                       long long *counts, int N, long V, int R, void *stream) {
    MVD_REQUIRE(logits && target && counts, "sigmoid_counts: null pointer");
    MVD_REQUIRE(N > 0 && N <= 65535 && V > 0 && R >= 1 && R <= RKMAX, "sigmoid_counts: bad shape (1 <= R <= 8 heads)");
    LabelLut lut;
    int TP;
    if (int rc = region_form("sigmoid_counts", target_form, lut_host, R, lut, TP)) return rc;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(counts, 0, sizeof(long long) * R * 3, s) != hipSuccess) {
        set_error("sigmoid_counts: memset failed");
        return 1;
    }
    const long bx = rgrid_for(V, rcap_per_n(1024, N));
    unsigned long long *c = reinterpret_cast<unsigned long long *>(counts);
    if (target_form == 0)
        hipLaunchKernelGGL(k_sigmoid_counts<false>, dim3(bx, N), dim3(256), 0, s, logits, target, lut, c, V, R, TP);
    else
        hipLaunchKernelGGL(k_sigmoid_counts<true>, dim3(bx, N), dim3(256), 0, s, logits, target, lut, c, V, R, TP);
    return check_launch("sigmoid_counts");
}

int mvd_argmax_counts_masked(const float *logits, const float *target, long long *counts, int N, long V, int K,
                             int ignore_label, void *stream) {
    MVD_REQUIRE(logits && target && counts, "argmax_counts_masked: null pointer");
    MVD_REQUIRE(N > 0 && N <= 65535 && V > 0 && K >= 1 && K <= RKMAX, "argmax_counts_masked: bad shape");
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(counts, 0, sizeof(long long) * K * 3, s) != hipSuccess) {
        set_error("argmax_counts_masked: memset failed");
        return 1;
    }
    const long bx = rgrid_for(V, rcap_per_n(1024, N));
    hipLaunchKernelGGL(k_argmax_counts_masked, dim3(bx, N), dim3(256), 0, s, logits, target,
                       reinterpret_cast<unsigned long long *>(counts), V, K, ignore_label);
    return check_launch("argmax_counts_masked");
}

int mvd_seg_to_regions(const float *seg, const uint32_t *lut_host, float *planes, int N, long V, int R, int with_ignore,
                       void *stream) {
    MVD_REQUIRE(seg && planes, "seg_to_regions: null pointer");
    MVD_REQUIRE(N > 0 && N <= 65535 && V > 0 && R >= 1 && R <= 31, "seg_to_regions: bad shape (1 <= R <= 31 regions)");
    LabelLut lut;
    int TP;
    if (int rc = region_form("seg_to_regions", 0, lut_host, R, lut, TP)) return rc;
    TP = R + (with_ignore ? 1 : 0);
    const long bx = rgrid_for(V, rcap_per_n(4096, N));
    hipLaunchKernelGGL(k_seg_to_regions, dim3(bx, N), dim3(256), 0, as_stream(stream), seg, lut, planes, V, R, TP);
    return check_launch("seg_to_regions");
}
}
