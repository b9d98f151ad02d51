// Segmentation export and evaluation after sliding-window inference (the tail of perform_actual_validation,
// nnUNetTrainer.py:1135-1260): resample the K logit planes to the shape before resampling, softmax / argmax, paste into
// the pre-crop volume and undo the plans' transpose -- one gather pass, the K x (D,H,W) float tensor of the argmax path
// is never written -- and the TP/FP/FN/TN counts of compute_metrics (evaluate_predictions.py:70-121).
//
// The kernels walk the OUTPUT buffer linearly (it is contiguous in the original axis order), so neighbouring lanes store
// neighbouring bytes whatever transpose_backward is; the permutation only changes which logits a lane gathers, and those
// go through the caches.  Every output byte has one writer, outside the bbox included: deterministic by construction.
#include "common.h"

namespace mvd {

struct ExportGeom {
    int K, d, h, w;   // logits [K][d][h][w]
    int nz, ny, nx;   // resampled size per network axis (== table lengths, tables concatenated z | y | x)
    int fz, fy, fx;   // pre-crop volume per network axis
    int lz, ly, lx;   // lower bbox corner per network axis
    int jz, jy, jx;   // OUTPUT axis that holds network axis z / y / x
    int O1, O2;       // output extents of the two inner output axes
};

struct Taps {
    size_t z0, z1, y0, y1;
    int x0, x1;
    float wz, wy, wx;
};

__device__ __forceinline__ int pick(int j, int a0, int a1, int a2) { return j == 0 ? a0 : (j == 1 ? a1 : a2); }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ float lerp(float a, float b, float t) { return fmaf(t, b - a, a); }

// false: the output voxel (a0,a1,a2) lies outside the bbox.  Table indices are clamped to the logits' extent here, so a
// wrong table can give a wrong value but never an out-of-bounds load.
__device__ __forceinline__ bool export_taps(const ExportGeom &g, const int *__restrict__ i0, const int *__restrict__ i1,
                                            const float *__restrict__ tw, int a0, int a1, int a2, Taps &t) {
    const int qz = pick(g.jz, a0, a1, a2) - g.lz, qy = pick(g.jy, a0, a1, a2) - g.ly, qx = pick(g.jx, a0, a1, a2) - g.lx;
    if ((unsigned)qz >= (unsigned)g.nz || (unsigned)qy >= (unsigned)g.ny || (unsigned)qx >= (unsigned)g.nx) return false;
    const int ey = g.nz + qy, ex = g.nz + g.ny + qx;
    const size_t hw = (size_t)g.h * g.w;
    t.z0 = (size_t)clampi(i0[qz], g.d - 1) * hw;
    t.z1 = (size_t)clampi(i1[qz], g.d - 1) * hw;
    t.y0 = (size_t)clampi(i0[ey], g.h - 1) * g.w;
    t.y1 = (size_t)clampi(i1[ey], g.h - 1) * g.w;
    t.x0 = clampi(i0[ex], g.w - 1);
    t.x1 = clampi(i1[ex], g.w - 1);
    t.wz = tw[qz];
    t.wy = tw[ey];
    t.wx = tw[ex];
    return true;
}

// one channel at one output voxel: fp32 lerps along W, then H, then D
__device__ __forceinline__ float export_interp(const float *__restrict__ p, const Taps &t) {
    const float a = lerp(p[t.z0 + t.y0 + t.x0], p[t.z0 + t.y0 + t.x1], t.wx);
    const float b = lerp(p[t.z0 + t.y1 + t.x0], p[t.z0 + t.y1 + t.x1], t.wx);
    const float c = lerp(p[t.z1 + t.y0 + t.x0], p[t.z1 + t.y0 + t.x1], t.wx);
    const float e = lerp(p[t.z1 + t.y1 + t.x0], p[t.z1 + t.y1 + t.x1], t.wx);
    return lerp(lerp(a, b, t.wy), lerp(c, e, t.wy), t.wz);
}

// Four consecutive output bytes per lane, one dword store (the output base is 4-byte aligned, total = all output voxels).
__global__ void __launch_bounds__(256) k_export_resize_argmax_u8(const float *__restrict__ logits, uint8_t *__restrict__ out,
                                                                 const int *__restrict__ i0, const int *__restrict__ i1,
                                                                 const float *__restrict__ tw, ExportGeom g, long total) {
    const long nquad = (total + 3) >> 2;
    const size_t dhw = (size_t)g.d * g.h * g.w;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += (long)gridDim.x * blockDim.x) {
        const long lin = q << 2;
        long r = lin / g.O2;
        int a2 = (int)(lin - r * g.O2);
        int a0 = (int)(r / g.O1);
        int a1 = (int)(r - (long)a0 * g.O1);
        const int nv = total - lin < 4 ? (int)(total - lin) : 4;
        unsigned pack = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j < nv) {
                Taps t;
                unsigned best = 0;
                if (export_taps(g, i0, i1, tw, a0, a1, a2, t)) {
                    float vmax = export_interp(logits, t);
                    for (int k = 1; k < g.K; k++) {
                        const float v = export_interp(logits + (size_t)k * dhw, t);
                        if (v > vmax) {  // strict: the first index wins an exact tie, as argmax does
                            vmax = v;
                            best = (unsigned)k;
                        }
                    }
                }
                pack |= best << (8 * j);
                if (++a2 == g.O2) {
                    a2 = 0;
                    if (++a1 == g.O1) {
                        a1 = 0;
                        ++a0;
                    }
                }
            }
        }
        if (nv == 4) {
            *reinterpret_cast<unsigned *>(out + lin) = pack;
        } else {
            for (int j = 0; j < nv; j++) out[lin + j] = (uint8_t)(pack >> (8 * j));
        }
    }
}

// One output voxel per lane, K float planes of `total` voxels.  softmax != 0: max, then exp(v - max) stored and summed,
// then the lane divides what it stored (fp32, k ascending); outside the bbox plane 0 is 1.  softmax == 0: the
// interpolated logits themselves, 0 outside.  The interpolation is evaluated twice rather than kept in K registers.
__global__ void __launch_bounds__(256) k_export_resize_f32(const float *__restrict__ logits, float *__restrict__ out,
                                                           const int *__restrict__ i0, const int *__restrict__ i1,
                                                           const float *__restrict__ tw, ExportGeom g, long total,
                                                           int softmax) {
    const size_t dhw = (size_t)g.d * g.h * g.w;
    for (long lin = (long)blockIdx.x * blockDim.x + threadIdx.x; lin < total; lin += (long)gridDim.x * blockDim.x) {
        const long r = lin / g.O2;
        const int a2 = (int)(lin - r * g.O2);
        const int a0 = (int)(r / g.O1);
        const int a1 = (int)(r - (long)a0 * g.O1);
        Taps t;
        if (!export_taps(g, i0, i1, tw, a0, a1, a2, t)) {
            for (int k = 0; k < g.K; k++) out[(size_t)k * total + lin] = (softmax && k == 0) ? 1.f : 0.f;
            continue;
        }
        if (!softmax) {
            for (int k = 0; k < g.K; k++) out[(size_t)k * total + lin] = export_interp(logits + (size_t)k * dhw, t);
            continue;
        }
        float vmax = export_interp(logits, t);
        for (int k = 1; k < g.K; k++) vmax = fmaxf(vmax, export_interp(logits + (size_t)k * dhw, t));
        float sum = 0.f;
        for (int k = 0; k < g.K; k++) {
            const float e = expf(export_interp(logits + (size_t)k * dhw, t) - vmax);
            out[(size_t)k * total + lin] = e;
            sum += e;
        }
        for (int k = 0; k < g.K; k++) out[(size_t)k * total + lin] = out[(size_t)k * total + lin] / sum;
    }
}

// ---------------------------------------------------------------------------------------------------- region export
// Region-based labels (label_handling.py:163-171): the segmentation starts at 0 and, head after head in
// regions_class_order order, voxels whose head is "on" take that head's label -- the last matching head wins.  A head is
// on iff its interpolated logit is > 0, i.e. sigma(z) > 0.5 in exact arithmetic (see mvdseg_hip.h).  Same tables, lerp
// order and one-writer linear walk as k_export_resize_argmax_u8.
struct RegionOrder {
    int c[8];
};

__global__ void __launch_bounds__(256) k_export_resize_regions_u8(const float *__restrict__ logits, uint8_t *__restrict__ out,
                                                                  const int *__restrict__ i0, const int *__restrict__ i1,
                                                                  const float *__restrict__ tw, ExportGeom g, long total,
                                                                  RegionOrder ord) {
    const long nquad = (total + 3) >> 2;
    const size_t dhw = (size_t)g.d * g.h * g.w;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += (long)gridDim.x * blockDim.x) {
        const long lin = q << 2;
        long r = lin / g.O2;
        int a2 = (int)(lin - r * g.O2);
        int a0 = (int)(r / g.O1);
        int a1 = (int)(r - (long)a0 * g.O1);
        const int nv = total - lin < 4 ? (int)(total - lin) : 4;
        unsigned pack = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j < nv) {
                Taps t;
                unsigned label = 0;
                if (export_taps(g, i0, i1, tw, a0, a1, a2, t)) {
#pragma unroll
                    for (int k = 0; k < 8; k++)  // static index into the by-value order (no run-time-indexed kernel argument)
                        if (k < g.K && export_interp(logits + (size_t)k * dhw, t) > 0.f) label = (unsigned)ord.c[k];
                }
                pack |= label << (8 * j);
                if (++a2 == g.O2) {
                    a2 = 0;
                    if (++a1 == g.O1) {
                        a1 = 0;
                        ++a0;
                    }
                }
            }
        }
        if (nv == 4) {
            *reinterpret_cast<unsigned *>(out + lin) = pack;
        } else {
            for (int j = 0; j < nv; j++) out[lin + j] = (uint8_t)(pack >> (8 * j));
        }
    }
}

// apply_nonlin = sigmoid: 1 / (1 + exp(-z)) of the interpolated logits, every plane 0 outside the bbox (no probs[0] = 1:
// label_handling.py:204-205)
__global__ void __launch_bounds__(256) k_export_resize_sigmoid_f32(const float *__restrict__ logits, float *__restrict__ out,
                                                                   const int *__restrict__ i0, const int *__restrict__ i1,
                                                                   const float *__restrict__ tw, ExportGeom g, long total) {
    const size_t dhw = (size_t)g.d * g.h * g.w;
    for (long lin = (long)blockIdx.x * blockDim.x + threadIdx.x; lin < total; lin += (long)gridDim.x * blockDim.x) {
        const long r = lin / g.O2;
        const int a2 = (int)(lin - r * g.O2);
        const int a0 = (int)(r / g.O1);
        const int a1 = (int)(r - (long)a0 * g.O1);
        Taps t;
        const bool in = export_taps(g, i0, i1, tw, a0, a1, a2, t);
        for (int k = 0; k < g.K; k++)
            out[(size_t)k * total + lin] = in ? 1.0f / (1.0f + expf(-export_interp(logits + (size_t)k * dhw, t))) : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------- ensemble export
// DESIGN 31.  M members (their own logits extent and tables) onto ONE output geometry: per output voxel and member the K
// logits are interpolated (export_taps / export_interp), soft-maxed with the operations of k_export_resize_f32 (max,
// expf(v - max), sum with k ascending, e / sum) and added to K register accumulators, members ascending; mean = acc / M
// (a division; none for M == 1), argmax with a strict >.  K is a template parameter and every k loop is unrolled, so that
// v[] and acc[] stay in registers; the member tables are a by-value argument read with a wave-uniform index.
constexpr int ENS_MMAX = 8;
constexpr int ENS_KMAX = 8;

struct EnsembleMembers {
    const float *logits[ENS_MMAX];
    const int *i0[ENS_MMAX];
    const int *i1[ENS_MMAX];
    const float *tw[ENS_MMAX];
    int d[ENS_MMAX], h[ENS_MMAX], w[ENS_MMAX];
};

// g: the shared output geometry (its d / h / w are filled per member).  PROB: also the fp32 mean planes [K][total].
template <int K, bool PROB>
__global__ void __launch_bounds__(256) k_export_ensemble(EnsembleMembers mem, int M, uint8_t *__restrict__ out,
                                                         float *__restrict__ mean, ExportGeom g, long total) {
    const long nquad = (total + 3) >> 2;
    const float fM = (float)M;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += (long)gridDim.x * blockDim.x) {
        const long lin = q << 2;
        long r = lin / g.O2;
        int a2 = (int)(lin - r * g.O2);
        int a0 = (int)(r / g.O1);
        int a1 = (int)(r - (long)a0 * g.O1);
        const int nv = total - lin < 4 ? (int)(total - lin) : 4;
        unsigned pack = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j < nv) {
                float acc[K];
#pragma unroll
                for (int k = 0; k < K; k++) acc[k] = k == 0 ? 1.f : 0.f;  // outside the bbox: channel 0 is 1
                bool in = false;
                for (int m = 0; m < M; m++) {
                    ExportGeom gm = g;
                    gm.d = mem.d[m];
                    gm.h = mem.h[m];
                    gm.w = mem.w[m];
                    Taps t;
                    in = export_taps(gm, mem.i0[m], mem.i1[m], mem.tw[m], a0, a1, a2, t);  // the same answer for every m
                    if (!in) break;
                    const float *__restrict__ p = mem.logits[m];
                    const size_t dhw = (size_t)gm.d * gm.h * gm.w;
                    float v[K];
#pragma unroll
                    for (int k = 0; k < K; k++) v[k] = export_interp(p + (size_t)k * dhw, t);
                    float vmax = v[0];
#pragma unroll
                    for (int k = 1; k < K; k++) vmax = fmaxf(vmax, v[k]);
                    float sum = 0.f;
#pragma unroll
                    for (int k = 0; k < K; k++) {
                        v[k] = expf(v[k] - vmax);
                        sum += v[k];
                    }
#pragma unroll
                    for (int k = 0; k < K; k++) {
                        const float pk = v[k] / sum;
                        acc[k] = m == 0 ? pk : acc[k] + pk;  // avg = p_0; avg += p_m
                    }
                }
                unsigned best = 0;
                if (in) {
                    if (M > 1) {
#pragma unroll
                        for (int k = 0; k < K; k++) acc[k] = acc[k] / fM;
                    }
                    float vbest = acc[0];
#pragma unroll
                    for (int k = 1; k < K; k++) {
                        if (acc[k] > vbest) {  // strict: the first index wins an exact tie
                            vbest = acc[k];
                            best = (unsigned)k;
                        }
                    }
                }
                if (PROB) {
#pragma unroll
                    for (int k = 0; k < K; k++) mean[(size_t)k * total + lin + j] = acc[k];
                }
                pack |= best << (8 * j);
                if (++a2 == g.O2) {
                    a2 = 0;
                    if (++a1 == g.O1) {
                        a1 = 0;
                        ++a0;
                    }
                }
            }
        }
        if (nv == 4) {
            *reinterpret_cast<unsigned *>(out + lin) = pack;
        } else {
            for (int j = 0; j < nv; j++) out[lin + j] = (uint8_t)(pack >> (8 * j));
        }
    }
}

// The stored-probabilities route (ensemble.py:17-29): avg = p_0; avg += p_m (m ascending); avg /= M; argmax with a strict >.
// M volumes [K][n] in, uint8 labels and (mean != nullptr) the fp32 mean [K][n] out.  Four voxels per lane: VEC (n % 4 == 0
// and every base 16-byte aligned) through 16-byte loads and stores, otherwise scalar; the labels leave as one dword per
// quad where seg is 4-byte aligned (seg4) and the quad is whole.
struct MeanMembers {
    const float *p[ENS_MMAX];
};

template <int K, bool VEC>
__global__ void __launch_bounds__(256) k_ensemble_mean_argmax(MeanMembers mem, int M, long n, uint8_t *__restrict__ seg,
                                                              float *__restrict__ mean, int seg4) {
    const long nquad = (n + 3) >> 2;
    const float fM = (float)M;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += (long)gridDim.x * blockDim.x) {
        const long lin = q << 2;
        const int nv = VEC ? 4 : (n - lin < 4 ? (int)(n - lin) : 4);
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        unsigned pack = 0;
#pragma unroll
        for (int k = 0; k < K; k++) {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            for (int m = 0; m < M; m++) {
                const float *__restrict__ p = mem.p[m] + (size_t)k * n + lin;
                float x[4] = {0.f, 0.f, 0.f, 0.f};
                if (VEC) {
                    const float4 f = *reinterpret_cast<const float4 *>(p);
                    x[0] = f.x; x[1] = f.y; x[2] = f.z; x[3] = f.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (j < nv) x[j] = p[j];
                }
#pragma unroll
                for (int j = 0; j < 4; j++) a[j] = m == 0 ? x[j] : a[j] + x[j];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                a[j] = a[j] / fM;
                if (k == 0 || a[j] > best[j]) {  // strict: the first index wins an exact tie
                    if (k != 0) pack = (pack & ~(0xffu << (8 * j))) | ((unsigned)k << (8 * j));
                    best[j] = a[j];
                }
            }
            if (mean) {
                float *__restrict__ o = mean + (size_t)k * n + lin;
                if (VEC) {
                    *reinterpret_cast<float4 *>(o) = make_float4(a[0], a[1], a[2], a[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (j < nv) o[j] = a[j];
                }
            }
        }
        if (nv == 4 && seg4) {
            *reinterpret_cast<unsigned *>(seg + lin) = pack;
        } else {
            for (int j = 0; j < nv; j++) seg[lin + j] = (uint8_t)(pack >> (8 * j));
        }
    }
}

// ---------------------------------------------------------------------------------------------------- confusion counts
struct RegionLut {
    uint32_t m[256];  // bit r of m[label]: label belongs to label set r
};

constexpr int CONF_RC = 4;                 // label sets per blockIdx.y (their counters live in registers)
constexpr int CONF_NV = 3 * CONF_RC + 1;   // tp, fp, fn per set + the valid voxels

struct ConfAcc {
    unsigned c[CONF_NV];
};

__device__ __forceinline__ void conf_add(ConfAcc &acc, const uint32_t *lut, int r0, int p, int gt, int has_ignore,
                                         int ignore) {
    const unsigned valid = (has_ignore && gt == ignore) ? 0u : 1u;
    const unsigned mp = lut[p] >> r0;
    const unsigned mg = ((unsigned)gt < 256u ? lut[gt] : 0u) >> r0;
#pragma unroll
    for (int j = 0; j < CONF_RC; j++) {
        const unsigned bp = (mp >> j) & 1u, bg = (mg >> j) & 1u;
        acc.c[3 * j + 0] += valid & bp & bg;
        acc.c[3 * j + 1] += valid & bp & (bg ^ 1u);
        acc.c[3 * j + 2] += valid & (bp ^ 1u) & bg;
    }
    acc.c[3 * CONF_RC] += valid;
}

// pred uint8, gt uint8 (GT16 = false) or int16 (GT16 = true); 16 voxels per lane and iteration through 16-byte loads.
// Integer sums only: per-lane uint32 (grid sized so that no lane sees 2^32 voxels), 64-bit from the wave reduction on, one
// integer atomic per counter and block.  counts[r] = {TP, FP, FN, TN}, zeroed by the host side before the launch.
template <bool GT16>
__global__ void __launch_bounds__(256) k_seg_confusion_counts(const uint8_t *__restrict__ pred, const void *__restrict__ gtv,
                                                              long n, RegionLut lutv, int R, int has_ignore, int ignore,
                                                              unsigned long long *__restrict__ counts) {
    __shared__ uint32_t lut[256];
    __shared__ unsigned long long red[4][CONF_NV];
    lut[threadIdx.x] = lutv.m[threadIdx.x];  // blockDim.x == 256
    __syncthreads();
    const int r0 = blockIdx.y * CONF_RC;
    ConfAcc acc;
#pragma unroll
    for (int i = 0; i < CONF_NV; i++) acc.c[i] = 0;
    const long n16 = n >> 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) {
        union {
            uint4 v;
            uint8_t b[16];
        } p;
        p.v = reinterpret_cast<const uint4 *>(pred)[i];
        if (GT16) {
            union {
                uint4 v[2];
                int16_t s[16];
            } gq;
            gq.v[0] = reinterpret_cast<const uint4 *>(gtv)[2 * i];
            gq.v[1] = reinterpret_cast<const uint4 *>(gtv)[2 * i + 1];
#pragma unroll
            for (int j = 0; j < 16; j++) conf_add(acc, lut, r0, p.b[j], gq.s[j], has_ignore, ignore);
        } else {
            union {
                uint4 v;
                uint8_t b[16];
            } gq;
            gq.v = reinterpret_cast<const uint4 *>(gtv)[i];
#pragma unroll
            for (int j = 0; j < 16; j++) conf_add(acc, lut, r0, p.b[j], gq.b[j], has_ignore, ignore);
        }
    }
    if (blockIdx.x == 0) {  // the n % 16 voxels behind the last whole chunk
        const long i = (n16 << 4) + threadIdx.x;
        if (threadIdx.x < 16 && i < n) {
            const int gt = GT16 ? (int)reinterpret_cast<const int16_t *>(gtv)[i] : (int)reinterpret_cast<const uint8_t *>(gtv)[i];
            conf_add(acc, lut, r0, pred[i], gt, has_ignore, ignore);
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < CONF_NV; i++) {
        unsigned long long v = acc.c[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) red[wid][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < CONF_RC && r0 + (int)threadIdx.x < R) {
        const int j = threadIdx.x;
        unsigned long long s[4] = {0, 0, 0, 0};
        for (int w = 0; w < 4; w++) {
            s[0] += red[w][3 * j + 0];
            s[1] += red[w][3 * j + 1];
            s[2] += red[w][3 * j + 2];
            s[3] += red[w][3 * CONF_RC];
        }
        unsigned long long *o = counts + (size_t)(r0 + j) * 4;
        atomicAdd(o + 0, s[0]);
        atomicAdd(o + 1, s[1]);
        atomicAdd(o + 2, s[2]);
        atomicAdd(o + 3, s[3] - s[0] - s[1] - s[2]);
    }
}

}  // namespace mvd

using namespace mvd;

static int export_geom(const char *what, ExportGeom &g, int K, int d, int h, int w, int D, int H, int W, const int *full,
                       const int *lo, const int *perm, long *total) {
    MVD_REQUIRE(full && lo && perm, "%s: null shape argument", what);
    MVD_REQUIRE(K >= 1 && d > 0 && h > 0 && w > 0 && D > 0 && H > 0 && W > 0, "%s: empty shape", what);
    const int n[3] = {D, H, W};
    for (int a = 0; a < 3; a++)
        MVD_REQUIRE(full[a] > 0 && lo[a] >= 0 && n[a] <= full[a] && lo[a] <= full[a] - n[a],
                    "%s: bbox [%d, %d) outside the volume's axis %d of %d", what, lo[a], lo[a] + n[a], a, full[a]);
    int inv[3] = {-1, -1, -1};
    for (int j = 0; j < 3; j++) {
        MVD_REQUIRE(perm[j] >= 0 && perm[j] < 3 && inv[perm[j]] < 0, "%s: transpose_backward is not a permutation", what);
        inv[perm[j]] = j;
    }
    g.K = K; g.d = d; g.h = h; g.w = w;
    g.nz = D; g.ny = H; g.nx = W;
    g.fz = full[0]; g.fy = full[1]; g.fx = full[2];
    g.lz = lo[0]; g.ly = lo[1]; g.lx = lo[2];
    g.jz = inv[0]; g.jy = inv[1]; g.jx = inv[2];
    g.O1 = full[perm[1]];
    g.O2 = full[perm[2]];
    *total = (long)full[0] * full[1] * full[2];
    return 0;
}

static inline unsigned export_grid(long n) {
    long b = cdiv(n, 256);
    if (b > 262144) b = 262144;
    return (unsigned)(b < 1 ? 1 : b);
}

extern "C" {

int mvd_export_resize_argmax_u8(const float *logits, unsigned char *out, const int *idx0, const int *idx1,
                                const float *weight, int K, int d, int h, int w, int D, int H, int W, const int *full,
                                const int *lo, const int *perm, void *stream) {
    MVD_REQUIRE(logits && out && idx0 && idx1 && weight, "export_resize_argmax_u8: null pointer");
    MVD_REQUIRE(K <= 255, "export_resize_argmax_u8: %d channels do not fit a uint8 label", K);
    MVD_REQUIRE(((uintptr_t)out & 3) == 0, "export_resize_argmax_u8: the output must be 4-byte aligned");
    ExportGeom g;
    long total = 0;
    if (int rc = export_geom("export_resize_argmax_u8", g, K, d, h, w, D, H, W, full, lo, perm, &total)) return rc;
    hipLaunchKernelGGL(k_export_resize_argmax_u8, dim3(export_grid(cdiv(total, 4))), dim3(256), 0, as_stream(stream), logits,
                       out, idx0, idx1, weight, g, total);
    return check_launch("export_resize_argmax_u8");
}

int mvd_export_resize_softmax_f32(const float *logits, float *out, const int *idx0, const int *idx1, const float *weight,
                                  int K, int d, int h, int w, int D, int H, int W, const int *full, const int *lo,
                                  const int *perm, int apply_softmax, void *stream) {
    MVD_REQUIRE(logits && out && idx0 && idx1 && weight, "export_resize_softmax_f32: null pointer");
    ExportGeom g;
    long total = 0;
    if (int rc = export_geom("export_resize_softmax_f32", g, K, d, h, w, D, H, W, full, lo, perm, &total)) return rc;
    hipLaunchKernelGGL(k_export_resize_f32, dim3(export_grid(total)), dim3(256), 0, as_stream(stream), logits, out, idx0,
                       idx1, weight, g, total, apply_softmax ? 1 : 0);
    return check_launch("export_resize_softmax_f32");
}

int mvd_export_resize_regions_u8(const float *logits, unsigned char *out, const int *idx0, const int *idx1,
                                 const float *weight, int R, int d, int h, int w, int D, int H, int W, const int *full,
                                 const int *lo, const int *perm, const int *class_order, void *stream) {
    MVD_REQUIRE(logits && out && idx0 && idx1 && weight && class_order, "export_resize_regions_u8: null pointer");
    MVD_REQUIRE(R >= 1 && R <= 8, "export_resize_regions_u8: 1..8 region heads");
    MVD_REQUIRE(((uintptr_t)out & 3) == 0, "export_resize_regions_u8: the output must be 4-byte aligned");
    RegionOrder ord;
    for (int i = 0; i < 8; i++) {
        ord.c[i] = i < R ? class_order[i] : 0;  // host array
        MVD_REQUIRE(ord.c[i] >= 0 && ord.c[i] <= 255, "export_resize_regions_u8: label %d does not fit a uint8", ord.c[i]);
    }
    ExportGeom g;
    long total = 0;
    if (int rc = export_geom("export_resize_regions_u8", g, R, d, h, w, D, H, W, full, lo, perm, &total)) return rc;
    hipLaunchKernelGGL(k_export_resize_regions_u8, dim3(export_grid(cdiv(total, 4))), dim3(256), 0, as_stream(stream), logits,
                       out, idx0, idx1, weight, g, total, ord);
    return check_launch("export_resize_regions_u8");
}

int mvd_export_resize_sigmoid_f32(const float *logits, float *out, const int *idx0, const int *idx1, const float *weight,
                                  int K, int d, int h, int w, int D, int H, int W, const int *full, const int *lo,
                                  const int *perm, void *stream) {
    MVD_REQUIRE(logits && out && idx0 && idx1 && weight, "export_resize_sigmoid_f32: null pointer");
    ExportGeom g;
    long total = 0;
    if (int rc = export_geom("export_resize_sigmoid_f32", g, K, d, h, w, D, H, W, full, lo, perm, &total)) return rc;
    hipLaunchKernelGGL(k_export_resize_sigmoid_f32, dim3(export_grid(total)), dim3(256), 0, as_stream(stream), logits, out,
                       idx0, idx1, weight, g, total);
    return check_launch("export_resize_sigmoid_f32");
}

#define ENS_LAUNCH(KK)                                                                                                  \
    case KK:                                                                                                            \
        if (mean)                                                                                                       \
            hipLaunchKernelGGL((k_export_ensemble<KK, true>), grid, dim3(256), 0, s, mem, M, out, mean, g, total);      \
        else                                                                                                            \
            hipLaunchKernelGGL((k_export_ensemble<KK, false>), grid, dim3(256), 0, s, mem, M, out, mean, g, total);     \
        break;

int mvd_export_ensemble_argmax_u8(const float *const *logits, const int *const *idx0, const int *const *idx1,
                                  const float *const *weight, const int *dims, int M, int K, int D, int H, int W,
                                  const int *full, const int *lo, const int *perm, unsigned char *out, float *mean,
                                  void *stream) {
    MVD_REQUIRE(M >= 1 && M <= ENS_MMAX, "export_ensemble_argmax_u8: %d members: 1..%d", M, ENS_MMAX);
    MVD_REQUIRE(K >= 2 && K <= ENS_KMAX, "export_ensemble_argmax_u8: %d heads: 2..%d (the per-lane accumulators)", K,
                ENS_KMAX);
    MVD_REQUIRE(logits && idx0 && idx1 && weight && dims && out, "export_ensemble_argmax_u8: null pointer");
    MVD_REQUIRE(((uintptr_t)out & 3) == 0, "export_ensemble_argmax_u8: the output must be 4-byte aligned");
    EnsembleMembers mem;
    memset(&mem, 0, sizeof(mem));
    for (int m = 0; m < M; m++) {  // host arrays
        MVD_REQUIRE(logits[m] && idx0[m] && idx1[m] && weight[m], "export_ensemble_argmax_u8: null pointer in member %d", m);
        MVD_REQUIRE(dims[3 * m] > 0 && dims[3 * m + 1] > 0 && dims[3 * m + 2] > 0,
                    "export_ensemble_argmax_u8: empty logits in member %d", m);
        mem.logits[m] = logits[m];
        mem.i0[m] = idx0[m];
        mem.i1[m] = idx1[m];
        mem.tw[m] = weight[m];
        mem.d[m] = dims[3 * m];
        mem.h[m] = dims[3 * m + 1];
        mem.w[m] = dims[3 * m + 2];
    }
    ExportGeom g;
    long total = 0;
    if (int rc = export_geom("export_ensemble_argmax_u8", g, K, mem.d[0], mem.h[0], mem.w[0], D, H, W, full, lo, perm, &total))
        return rc;
    hipStream_t s = as_stream(stream);
    const dim3 grid(export_grid(cdiv(total, 4)));
    switch (K) {
        ENS_LAUNCH(2) ENS_LAUNCH(3) ENS_LAUNCH(4) ENS_LAUNCH(5) ENS_LAUNCH(6) ENS_LAUNCH(7) ENS_LAUNCH(8)
    }
    return check_launch("export_ensemble_argmax_u8");
}
#undef ENS_LAUNCH

#define MEAN_LAUNCH(KK)                                                                                                 \
    case KK:                                                                                                            \
        if (vec)                                                                                                        \
            hipLaunchKernelGGL((k_ensemble_mean_argmax<KK, true>), grid, dim3(256), 0, s, mem, M, n, seg, mean, seg4);  \
        else                                                                                                            \
            hipLaunchKernelGGL((k_ensemble_mean_argmax<KK, false>), grid, dim3(256), 0, s, mem, M, n, seg, mean, seg4); \
        break;

int mvd_ensemble_mean_argmax(const float *const *probs, int M, int K, long n, unsigned char *seg, float *mean,
                             void *stream) {
    MVD_REQUIRE(M >= 1 && M <= ENS_MMAX, "ensemble_mean_argmax: %d members: 1..%d", M, ENS_MMAX);
    MVD_REQUIRE(K >= 1 && K <= ENS_KMAX, "ensemble_mean_argmax: %d channels: 1..%d", K, ENS_KMAX);
    MVD_REQUIRE(probs && seg, "ensemble_mean_argmax: null pointer");
    MVD_REQUIRE(n > 0 && n < (1L << 40), "ensemble_mean_argmax: bad voxel count");
    MeanMembers mem;
    memset(&mem, 0, sizeof(mem));
    uintptr_t bits = (uintptr_t)mean;
    for (int m = 0; m < M; m++) {  // host array
        MVD_REQUIRE(probs[m], "ensemble_mean_argmax: null pointer in member %d", m);
        MVD_REQUIRE(((uintptr_t)probs[m] & 3) == 0, "ensemble_mean_argmax: member %d is not 4-byte aligned", m);
        mem.p[m] = probs[m];
        bits |= (uintptr_t)probs[m];
    }
    MVD_REQUIRE(((uintptr_t)mean & 3) == 0, "ensemble_mean_argmax: the mean is not 4-byte aligned");
    const bool vec = (n & 3) == 0 && (bits & 15) == 0;
    const int seg4 = ((uintptr_t)seg & 3) == 0 ? 1 : 0;
    hipStream_t s = as_stream(stream);
    const dim3 grid(export_grid(cdiv(n, 4)));
    switch (K) {
        MEAN_LAUNCH(1) MEAN_LAUNCH(2) MEAN_LAUNCH(3) MEAN_LAUNCH(4) MEAN_LAUNCH(5) MEAN_LAUNCH(6) MEAN_LAUNCH(7) MEAN_LAUNCH(8)
    }
    return check_launch("ensemble_mean_argmax");
}
#undef MEAN_LAUNCH

int mvd_seg_confusion_counts(const unsigned char *pred, const void *gt, int gt_is_i16, long n, const int32_t *label_sets,
                             const int *set_sizes, int R, int has_ignore, int ignore_label, long long *counts,
                             void *stream) {
    MVD_REQUIRE(pred && gt && label_sets && set_sizes && counts, "seg_confusion_counts: null pointer");
    MVD_REQUIRE(n > 0 && n < (1L << 40), "seg_confusion_counts: bad voxel count");
    MVD_REQUIRE(R >= 1 && R <= 32, "seg_confusion_counts: 1..32 label sets");
    MVD_REQUIRE((((uintptr_t)pred | (uintptr_t)gt) & 15) == 0, "seg_confusion_counts: volumes must be 16-byte aligned");
    RegionLut lut;
    memset(&lut, 0, sizeof(lut));
    for (int r = 0; r < R; r++) {
        MVD_REQUIRE(set_sizes[r] >= 1 && set_sizes[r] <= 16, "seg_confusion_counts: 1..16 labels per set");
        for (int i = 0; i < set_sizes[r]; i++) {
            const int32_t l = label_sets[r * 16 + i];  // host array, [R][16]
            MVD_REQUIRE(l >= 0 && l <= 255, "seg_confusion_counts: label %d outside 0..255", (int)l);
            lut.m[l] |= 1u << r;
        }
    }
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(counts, 0, (size_t)R * 4 * sizeof(long long), s) != hipSuccess) {
        set_error("seg_confusion_counts: memset failed");
        return 1;
    }
    long bx = cdiv(n >> 4, 256);
    if (bx > 2048) bx = 2048;
    if (bx < 1) bx = 1;
    const dim3 grid((unsigned)bx, (unsigned)cdiv(R, CONF_RC));
    unsigned long long *c = reinterpret_cast<unsigned long long *>(counts);
    if (gt_is_i16)
        hipLaunchKernelGGL(k_seg_confusion_counts<true>, grid, dim3(256), 0, s, pred, gt, n, lut, R, has_ignore ? 1 : 0,
                           ignore_label, c);
    else
        hipLaunchKernelGGL(k_seg_confusion_counts<false>, grid, dim3(256), 0, s, pred, gt, n, lut, R, has_ignore ? 1 : 0,
                           ignore_label, c);
    return check_launch("seg_confusion_counts");
}
}
