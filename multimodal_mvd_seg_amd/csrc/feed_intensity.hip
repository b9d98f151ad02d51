// On-device intensity augmentations of the training feed: the transforms nnU-Net's default pipeline runs
// between SpatialTransform and MirrorTransform (nnUNetTrainer.py:719-736), plus MaskTransform.  The numeric cores are
// pinned to numpy / scipy.ndimage:
//   k_chan_stats_*        per-channel mean, std (ddof 0), min, max: fp64 sums, fixed two-level order, no atomics
//   k_intensity_apply     brightness (x *= m), contrast (clip((x - mean) f + mean, min, max)), the two gamma maps with
//                         retain_stats, and the low-res clip; statistics read from the device
//   k_gaussian_blur_axis  scipy.ndimage.gaussian_filter: one separable pass, reflect boundary (repeated reflection on
//                         short axes), normalised fp64 weights of radius int(4 sigma + 0.5)
//   k_gaussian_noise      x += sigma N(0, 1), N from Philox4x64-10 (numpy.random.Philox's stream) and Box-Muller
//   k_lowres_gather       zoom(order=0, mode='nearest', grid_mode=True) of the un-flipped patch, edge-padded by 12
//   k_mask_remove_label   MaskTransform (data = 0 where seg[0] < 0) and RemoveLabelTransform(-1, 0) in one pass
// Planar fp32 [C][D][H][W]; per-channel parameters travel by value in the kernel arguments (capturable calls).
#include "common.h"

namespace mvd {

constexpr int kMaxCh = 16;       // channels per call (per-channel tables are kernel arguments)
constexpr int kStatBlocks = 256; // partial-sum blocks per channel (first reduction level)

struct ChanF {
    float v[kMaxCh];
};

__device__ __forceinline__ bool chan_on(int mask, int c) { return (mask >> c) & 1; }

// y of augment_gamma on one voxel: z = x (or -x when inv), y = ((z - lo) / (r + 1e-7))^g (r + 1e-7) + lo with lo, r
// the min and the range of z.  st = {mean, std, min, max} of x.
__device__ __forceinline__ float gamma_y(float x, int inv, float g, const double *st) {
    const double lo = inv ? -st[3] : st[2];
    const double rr = (st[3] - st[2]) + 1e-7;
    const float z = inv ? -x : x;
    float b = (z - (float)lo) * (float)(1.0 / rr);
    b = b > 0.f ? b : 0.f;
    return powf(b, g) * (float)rr + (float)lo;
}

// ------------------------------------------------------------------------------------------------ statistics
// pre: 0 the channel itself, 2 / 3 the gamma map y of it (3: of -x), with the channel's stats in pre_st.
__global__ void __launch_bounds__(256) k_chan_stats_partial(const float *__restrict__ x, double *__restrict__ part,
                                                            long V, int chmask, int pre, ChanF g,
                                                            const double *__restrict__ pre_st) {
    __shared__ double sm[4][4];
    const int c = blockIdx.y;
    if (!chan_on(chmask, c)) return;
    const float *xc = x + c * V;
    const double *st = pre_st ? pre_st + 4 * c : nullptr;
    const float gc = g.v[c];
    double s = 0.0, ss = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (long)gridDim.x * blockDim.x) {
        float v = xc[i];
        if (pre) v = gamma_y(v, pre == 3, gc, st);
        s += v;
        ss += (double)v * v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        ss += __shfl_xor(ss, o, 64);
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sm[w][0] = s;
        sm[w][1] = ss;
        sm[w][2] = mn;
        sm[w][3] = mx;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        double r = sm[0][k];
        for (int j = 1; j < 4; ++j) r = k < 2 ? r + sm[j][k] : (k == 2 ? fmin(r, sm[j][k]) : fmax(r, sm[j][k]));
        part[((long)c * gridDim.x + blockIdx.x) * 4 + k] = r;
    }
}

// One 256-lane block per channel folds the kStatBlocks partials (lane i owns partial i) in a fixed order.
__global__ void __launch_bounds__(256) k_chan_stats_final(const double *__restrict__ part, double *__restrict__ stats,
                                                          long V, int chmask, int nb) {
    __shared__ double sm[4][4];
    const int c = blockIdx.x;
    if (!chan_on(chmask, c)) return;
    double s = 0.0, ss = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) {
        const double *p = part + ((long)c * nb + i) * 4;
        s += p[0];
        ss += p[1];
        mn = fmin(mn, p[2]);
        mx = fmax(mx, p[3]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        ss += __shfl_xor(ss, o, 64);
        mn = fmin(mn, __shfl_xor(mn, o, 64));
        mx = fmax(mx, __shfl_xor(mx, o, 64));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sm[w][0] = s;
        sm[w][1] = ss;
        sm[w][2] = mn;
        sm[w][3] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < 4; ++j) {
            sm[0][0] += sm[j][0];
            sm[0][1] += sm[j][1];
            sm[0][2] = fmin(sm[0][2], sm[j][2]);
            sm[0][3] = fmax(sm[0][3], sm[j][3]);
        }
        const double mean = sm[0][0] / (double)V;
        const double var = sm[0][1] / (double)V - mean * mean;
        stats[4 * c + 0] = mean;
        stats[4 * c + 1] = var > 0.0 ? sqrt(var) : 0.0;
        stats[4 * c + 2] = sm[0][2];
        stats[4 * c + 3] = sm[0][3];
    }
}

// ------------------------------------------------------------------------------------------------ pointwise
enum { kOpBrightness = 0, kOpContrast = 1, kOpGamma = 2, kOpGammaInv = 3, kOpClip = 4 };

// sa = stats of the channel {mean, std, min, max}; sb = stats of its gamma map y (gamma ops only).
__global__ void __launch_bounds__(256) k_intensity_apply(float *__restrict__ x, long V, int chmask, int op, ChanF prm,
                                                         const double *__restrict__ sa, const double *__restrict__ sb) {
    const int c = blockIdx.y;
    if (!chan_on(chmask, c)) return;
    float *xc = x + c * V;
    const float p = prm.v[c];
    const double *st = sa ? sa + 4 * c : nullptr;
    float a = 0.f, b = 0.f, lo = 0.f, hi = 0.f;
    if (op == kOpContrast) {
        a = (float)st[0];
        lo = (float)st[2];
        hi = (float)st[3];
    } else if (op == kOpClip) {
        lo = (float)st[2];
        hi = (float)st[3];
    } else if (op == kOpGamma || op == kOpGammaInv) {
        // out_z = (y - mean_y) / (std_y + 1e-8) * std_z + mean_z, z = x or -x (std_z = std_x, mean_z = +-mean_x)
        const double *sy = sb + 4 * c;
        a = (float)sy[0];
        b = (float)(st[1] / (sy[1] + 1e-8));
        lo = (float)(op == kOpGammaInv ? -st[0] : st[0]);
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (long)gridDim.x * blockDim.x) {
        const float v = xc[i];
        float r;
        if (op == kOpBrightness) {
            r = v * p;
        } else if (op == kOpContrast) {
            r = (v - a) * p + a;
            r = r < lo ? lo : (r > hi ? hi : r);
        } else if (op == kOpClip) {
            r = v < lo ? lo : (v > hi ? hi : v);
        } else {
            const float y = gamma_y(v, op == kOpGammaInv, p, st);
            r = (y - a) * b + lo;
            if (op == kOpGammaInv) r = -r;
        }
        xc[i] = r;
    }
}

// ------------------------------------------------------------------------------------------------ blur
struct BlurArgs {
    int ch[kMaxCh];       // selected channels
    int rad[kMaxCh];      // radius per selected channel (<= 4)
    float w[kMaxCh][5];   // w[k] = weight of offset +-k, normalised in fp64
};

// scipy 'reflect' (d c b a | a b c d | d c b a), repeated on lines shorter than the filter
__device__ __forceinline__ int reflect_index(int i, int n) {
    const int p = 2 * n;
    int m = i % p;
    m = m < 0 ? m + p : m;
    return m < n ? m : p - 1 - m;
}

// One axis of the separable filter for every selected channel; block row y = selected channel k.  in_sel / out_sel:
// the in / out tensor is indexed by the channel itself (x) rather than by k (the [nsel] scratch).
__global__ void __launch_bounds__(256) k_gaussian_blur_axis(const float *__restrict__ in, float *__restrict__ out,
                                                            int D, int H, int W, int axis, BlurArgs a, int in_sel,
                                                            int out_sel) {
    const int k = blockIdx.y;
    const long V = (long)D * H * W;
    const float *src = in + (in_sel ? a.ch[k] : k) * V;
    float *dst = out + (out_sel ? a.ch[k] : k) * V;
    const int r = a.rad[k];
    const float *w = a.w[k];
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        int i, n;
        long s;
        if (axis == 2) {
            i = (int)(v % W);
            n = W;
            s = 1;
        } else if (axis == 1) {
            i = (int)((v / W) % H);
            n = H;
            s = W;
        } else {
            i = (int)(v / ((long)H * W));
            n = D;
            s = (long)H * W;
        }
        const float *line = src + (v - (long)i * s);
        float acc = w[0] * line[(long)i * s];
        for (int t = 1; t <= r; ++t)
            acc += w[t] * (line[(long)reflect_index(i - t, n) * s] + line[(long)reflect_index(i + t, n) * s]);
        dst[v] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ noise
// (Philox4x64-10: common.h)
// One N(0, 1) per 64-bit word: u1 = (2 (w >> 41) + 1) 2^-24, u2 = (2 ((w >> 18) & (2^23 - 1)) + 1) 2^-24 (exact in
// fp32, both in (0, 1)), z = sqrt(-2 ln u1) cos(2 pi u2).
__device__ __forceinline__ float normal_of(unsigned long long w) {
    const float u1 = (float)(2u * (unsigned)(w >> 41) + 1u) * 5.9604644775390625e-8f;
    const float u2 = (float)(2u * (unsigned)((w >> 18) & 0x7FFFFFu) + 1u) * 5.9604644775390625e-8f;
    return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// Raw output k = c V + v (stored voxel v of channel c) drives that voxel; one lane per Philox block of 4 outputs.
__global__ void __launch_bounds__(256) k_gaussian_noise(float *__restrict__ x, long V, int C, int chmask,
                                                        unsigned long long k0, unsigned long long k1, float sigma) {
    const long total = (long)C * V;
    const long nblk = (total + 3) / 4;
    for (long b = (long)blockIdx.x * blockDim.x + threadIdx.x; b < nblk; b += (long)gridDim.x * blockDim.x) {
        unsigned long long w[4];
        philox4x64_10((unsigned long long)b + 1ull, k0, k1, w);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long k = 4 * b + j;
            if (k < total && chan_on(chmask, (int)(k / V))) x[k] += sigma * normal_of(w[j]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ low resolution
// scipy zoom(order=0, mode='nearest', grid_mode=True) source index of output o (n -> t), in scipy's own fp64 steps
// (cc = (o + 0.5) (n / t) - 0.5, then floor(cc + 0.5)), without FMA contraction so ties round as scipy rounds them.
__device__ __forceinline__ int zoom0_index(int o, int n, int t) {
#pragma clang fp contract(off)
    const double z = (double)n / (double)t;
    const double cc = ((double)o + 0.5) * z - 0.5;
    int i = (int)floor(cc + 0.5);
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// dpad[q] = d[clamp(q - pad)] with d = zoom0 of the UN-flipped channel x (stored mirrored on flip_mask): the edge-padded
// order-0 downsample that scipy's order-3 zoom prefilters (_prepad_for_spline_filter, npad 12, mode 'nearest').
__global__ void __launch_bounds__(256) k_lowres_gather(const float *__restrict__ x, float *__restrict__ dpad, int D,
                                                       int H, int W, int td, int th, int tw, int pad, int flip_mask) {
    const int pd = td + 2 * pad, ph = th + 2 * pad, pw = tw + 2 * pad;
    const long total = (long)pd * ph * pw;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const int qx = (int)(q % pw), qy = (int)((q / pw) % ph), qz = (int)(q / ((long)pw * ph));
        const int uz = min(max(qz - pad, 0), td - 1), uy = min(max(qy - pad, 0), th - 1), ux = min(max(qx - pad, 0), tw - 1);
        int sz = zoom0_index(uz, D, td), sy = zoom0_index(uy, H, th), sx = zoom0_index(ux, W, tw);
        if (flip_mask & 1) sz = D - 1 - sz;
        if (flip_mask & 2) sy = H - 1 - sy;
        if (flip_mask & 4) sx = W - 1 - sx;
        dpad[q] = x[((long)sz * H + sy) * W + sx];
    }
}

// The in-plane form (SimulateLowResolutionTransform with ignore_axes=(0,), the dummy 2-D mode): axis 0 keeps its size and
// its index, dpad [D][th+2pad][tw+2pad] is padded on H and W only.
__global__ void __launch_bounds__(256) k_lowres_gather2d(const float *__restrict__ x, float *__restrict__ dpad, int D,
                                                         int H, int W, int th, int tw, int pad, int flip_mask) {
    const int ph = th + 2 * pad, pw = tw + 2 * pad;
    const long total = (long)D * ph * pw;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const int qx = (int)(q % pw), qy = (int)((q / pw) % ph), qz = (int)(q / ((long)pw * ph));
        const int uy = min(max(qy - pad, 0), th - 1), ux = min(max(qx - pad, 0), tw - 1);
        int sz = qz, sy = zoom0_index(uy, H, th), sx = zoom0_index(ux, W, tw);
        if (flip_mask & 1) sz = D - 1 - sz;
        if (flip_mask & 2) sy = H - 1 - sy;
        if (flip_mask & 4) sx = W - 1 - sx;
        dpad[q] = x[((long)sz * H + sy) * W + sx];
    }
}

// ------------------------------------------------------------------------------------------------ mask + RemoveLabel
__global__ void __launch_bounds__(256) k_mask_remove_label(float *__restrict__ data, float *__restrict__ seg, int C,
                                                           int Cs, long V, int chmask, int do_rep, float rep_from,
                                                           float rep_to) {
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        if (seg[v] < 0.f)
            for (int c = 0; c < C; ++c)
                if (chan_on(chmask, c)) data[c * V + v] = 0.f;
        if (do_rep)
            for (int c = 0; c < Cs; ++c)
                if (seg[c * V + v] == rep_from) seg[c * V + v] = rep_to;
    }
}

}  // namespace mvd

using namespace mvd;

static unsigned stride_grid(long n, long cap) {
    long b = cdiv(n, 256);
    if (b > cap) b = cap;
    return (unsigned)(b < 1 ? 1 : b);
}

static bool chan_ok(int C, int chmask) { return C > 0 && C <= kMaxCh && chmask >= 0 && chmask < (1 << C); }

static ChanF load_chan(const float *p, int C) {
    ChanF t = {};
    for (int c = 0; c < C; ++c) t.v[c] = p ? p[c] : 0.f;
    return t;
}

extern "C" {

size_t mvd_feed_stats_workspace_bytes(int C) { return (size_t)(C > 0 ? C : 0) * kStatBlocks * 4 * sizeof(double); }

int mvd_feed_channel_stats_f32(const float *x, double *stats, double *ws, int C, long V, int chmask, int pre_op,
                               const float *params, const double *pre_stats, void *stream) {
    MVD_REQUIRE(x && stats && ws, "feed_channel_stats_f32: null pointer");
    MVD_REQUIRE(chan_ok(C, chmask) && V > 0, "feed_channel_stats_f32: bad shape (1 <= C <= 16, V > 0)");
    MVD_REQUIRE(pre_op == 0 || pre_op == kOpGamma || pre_op == kOpGammaInv, "feed_channel_stats_f32: pre_op is 0, 2 or 3");
    MVD_REQUIRE(pre_op == 0 || (params && pre_stats), "feed_channel_stats_f32: the gamma map needs params and pre_stats");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_chan_stats_partial, dim3(kStatBlocks, C), dim3(256), 0, s, x, ws, V, chmask, pre_op,
                       load_chan(pre_op ? params : nullptr, C), pre_op ? pre_stats : nullptr);
    int e = check_launch("feed_channel_stats_f32");
    if (e) return e;
    hipLaunchKernelGGL(k_chan_stats_final, dim3(C), dim3(256), 0, s, ws, stats, V, chmask, kStatBlocks);
    return check_launch("feed_channel_stats_f32");
}

int mvd_feed_intensity_apply_f32(float *x, int C, long V, int chmask, int op, const float *params,
                                 const double *stats_a, const double *stats_b, void *stream) {
    MVD_REQUIRE(x, "feed_intensity_apply_f32: null pointer");
    MVD_REQUIRE(chan_ok(C, chmask) && V > 0, "feed_intensity_apply_f32: bad shape (1 <= C <= 16, V > 0)");
    MVD_REQUIRE(op >= kOpBrightness && op <= kOpClip, "feed_intensity_apply_f32: op is 0..4");
    MVD_REQUIRE(op == kOpClip || params, "feed_intensity_apply_f32: params required");
    MVD_REQUIRE(op == kOpBrightness || stats_a, "feed_intensity_apply_f32: stats_a required");
    MVD_REQUIRE((op != kOpGamma && op != kOpGammaInv) || stats_b, "feed_intensity_apply_f32: stats_b required");
    hipLaunchKernelGGL(k_intensity_apply, dim3(stride_grid(V, 1024), C), dim3(256), 0, as_stream(stream), x, V, chmask,
                       op, load_chan(params, C), stats_a, stats_b);
    return check_launch("feed_intensity_apply_f32");
}

int mvd_feed_gaussian_blur_f32(float *x, float *ws, int C, int D, int H, int W, const double *sigma, void *stream) {
    MVD_REQUIRE(x && ws && sigma, "feed_gaussian_blur_f32: null pointer");
    MVD_REQUIRE(C > 0 && C <= kMaxCh && D > 0 && H > 0 && W > 0, "feed_gaussian_blur_f32: bad shape (1 <= C <= 16)");
    MVD_REQUIRE((long)D * H * W < (1L << 40), "feed_gaussian_blur_f32: volume too large");
    BlurArgs a = {};
    int nsel = 0;
    for (int c = 0; c < C; ++c) {
        const double sg = sigma[c];
        if (!(sg > 0.0)) continue;  // channel not selected
        const int r = (int)(4.0 * sg + 0.5);
        MVD_REQUIRE(r <= 4, "feed_gaussian_blur_f32: sigma <= 1.1 (radius int(4 sigma + 0.5) <= 4)");
        double w[9], sum = 0.0;
        for (int t = -r; t <= r; ++t) sum += (w[t + r] = exp(-0.5 / (sg * sg) * (double)(t * t)));
        a.ch[nsel] = c;
        a.rad[nsel] = r;
        for (int t = 0; t <= r; ++t) a.w[nsel][t] = (float)(w[r + t] / sum);
        ++nsel;
    }
    if (nsel == 0) return 0;
    const long V = (long)D * H * W;
    float *t1 = ws, *t2 = ws + nsel * V;
    hipStream_t s = as_stream(stream);
    const dim3 grid(stride_grid(V, 1024), nsel);
    hipLaunchKernelGGL(k_gaussian_blur_axis, grid, dim3(256), 0, s, x, t1, D, H, W, 0, a, 1, 0);
    int e = check_launch("feed_gaussian_blur_f32");
    if (e) return e;
    hipLaunchKernelGGL(k_gaussian_blur_axis, grid, dim3(256), 0, s, t1, t2, D, H, W, 1, a, 0, 0);
    if ((e = check_launch("feed_gaussian_blur_f32"))) return e;
    hipLaunchKernelGGL(k_gaussian_blur_axis, grid, dim3(256), 0, s, t2, x, D, H, W, 2, a, 0, 1);
    return check_launch("feed_gaussian_blur_f32");
}

int mvd_feed_gaussian_noise_f32(float *x, int C, long V, int chmask, uint64_t key0, uint64_t key1, float sigma,
                                void *stream) {
    MVD_REQUIRE(x, "feed_gaussian_noise_f32: null pointer");
    MVD_REQUIRE(chan_ok(C, chmask) && V > 0, "feed_gaussian_noise_f32: bad shape (1 <= C <= 16, V > 0)");
    const long nblk = cdiv((long)C * V, 4);
    hipLaunchKernelGGL(k_gaussian_noise, dim3(stride_grid(nblk, 2048)), dim3(256), 0, as_stream(stream), x, V, C,
                       chmask, (unsigned long long)key0, (unsigned long long)key1, sigma);
    return check_launch("feed_gaussian_noise_f32");
}

int mvd_feed_lowres_gather_f32(const float *x, float *dpad, int D, int H, int W, int td, int th, int tw, int pad,
                               int flip_mask, void *stream) {
    MVD_REQUIRE(x && dpad, "feed_lowres_gather_f32: null pointer");
    MVD_REQUIRE(D > 0 && H > 0 && W > 0 && td > 0 && th > 0 && tw > 0 && pad >= 0, "feed_lowres_gather_f32: bad shape");
    MVD_REQUIRE(flip_mask >= 0 && flip_mask < 8, "feed_lowres_gather_f32: flip_mask is a 3-bit axis mask");
    MVD_REQUIRE(D < (1 << 20) && H < (1 << 20) && W < (1 << 20) && td < (1 << 20) && th < (1 << 20) && tw < (1 << 20) &&
                    pad <= 64,
                "feed_lowres_gather_f32: bad shape");
    const long total = (long)(td + 2 * pad) * (th + 2 * pad) * (tw + 2 * pad);
    hipLaunchKernelGGL(k_lowres_gather, dim3(stride_grid(total, 4096)), dim3(256), 0, as_stream(stream), x, dpad, D, H,
                       W, td, th, tw, pad, flip_mask);
    return check_launch("feed_lowres_gather_f32");
}

int mvd_feed_lowres_gather2d_f32(const float *x, float *dpad, int D, int H, int W, int th, int tw, int pad,
                                 int flip_mask, void *stream) {
    MVD_REQUIRE(x && dpad, "feed_lowres_gather2d_f32: null pointer");
    MVD_REQUIRE(D > 0 && H > 0 && W > 0 && th > 0 && tw > 0 && pad >= 0, "feed_lowres_gather2d_f32: bad shape");
    MVD_REQUIRE(flip_mask >= 0 && flip_mask < 8, "feed_lowres_gather2d_f32: flip_mask is a 3-bit axis mask");
    MVD_REQUIRE(D < (1 << 20) && H < (1 << 20) && W < (1 << 20) && th < (1 << 20) && tw < (1 << 20) && pad <= 64,
                "feed_lowres_gather2d_f32: bad shape");
    const long total = (long)D * (th + 2 * pad) * (tw + 2 * pad);
    hipLaunchKernelGGL(k_lowres_gather2d, dim3(stride_grid(total, 4096)), dim3(256), 0, as_stream(stream), x, dpad, D, H,
                       W, th, tw, pad, flip_mask);
    return check_launch("feed_lowres_gather2d_f32");
}

int mvd_feed_mask_remove_label(float *data, float *seg, int C, int Cs, long V, int chmask, int replace,
                               int replace_from, int replace_to, void *stream) {
    MVD_REQUIRE(data && seg, "feed_mask_remove_label: null pointer");
    MVD_REQUIRE(chan_ok(C, chmask) && Cs > 0 && V > 0, "feed_mask_remove_label: bad shape (1 <= C <= 16)");
    hipLaunchKernelGGL(k_mask_remove_label, dim3(stride_grid(V, 4096)), dim3(256), 0, as_stream(stream), data, seg, C,
                       Cs, V, chmask, replace ? 1 : 0, (float)replace_from, (float)replace_to);
    return check_launch("feed_mask_remove_label");
}
}
