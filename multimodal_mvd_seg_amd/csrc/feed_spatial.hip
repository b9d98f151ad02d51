// On-device SpatialTransform of the training feed: the rotation / scaling that nnU-Net's default pipeline
// applies to the initial patch (nnUNetTrainer.py:703-714, batchgenerators augment_spatial with order_data=3,
// order_seg=1, border mode 'constant').  The resampling is pinned to scipy.ndimage:
//   k_bspline_prefilter_*  == spline_filter1d(order=3, mode='mirror') per axis (gain 6, pole z = sqrt(3) - 2, scipy's
//                             mirror initialisation of the causal and anti-causal passes; a length-1 line is unchanged)
//   k_spatial_warp_data    == map_coordinates(order=3, mode='constant', cval) on the prefiltered patch: 4x4x4 cubic
//                             B-spline taps at floor(p)-1 .. floor(p)+2, tap indices mirrored, cval outside [0, n-1]
//   k_spatial_warp_seg     == batchgenerators interpolate_img(order=1, cval=-1, is_seg=True): per-label linear
//                             indicator, the largest label reaching 0.5 wins, 0 elsewhere
//   k_spatial_warp2d_*     == the same two resamplers per slice (c, z) under one in-plane map: the dummy 2-D mode of
//                             anisotropic plans (Convert3DTo2DTransform); 4x4 cubic / 4 linear taps
// Planar fp32 [C][D][H][W].  The per-sample coordinate map is p = A (o - (f-1)/2) + off, A and off by value.
#include "common.h"

namespace mvd {

constexpr float kPole = -0.26794919243112270f;  // sqrt(3) - 2
constexpr int kInitTerms = 32;                   // |z|^32 < 1e-18: the causal sum is exact in fp32 beyond this

// In-place cubic B-spline prefilter of one line c[0], c[s], ... c[(n-1)s] (scipy ni_splines.c, mirror boundary).
template <typename P>
__device__ __forceinline__ void bspline3_line(P c, int n, long s) {
    if (n < 2) return;
    const float z = kPole;
    // causal init: c0 = sum_i z^i (x_i + z^(n-1) x_(n-1-i)) / (1 - z^(2n-2)), x already multiplied by the gain 6
    const float zn1 = n - 1 < kInitTerms ? powf(-z, (float)(n - 1)) * (((n - 1) & 1) ? -1.f : 1.f) : 0.f;
    float c0 = 6.f * (c[0] + zn1 * c[(long)(n - 1) * s]);
    float zi = z;
    const int m = n - 1 < kInitTerms ? n - 1 : kInitTerms;
    for (int i = 1; i < m; ++i) {
        c0 += zi * 6.f * (c[(long)i * s] + zn1 * c[(long)(n - 1 - i) * s]);
        zi *= z;
    }
    float prev = c0 / (1.f - zn1 * zn1);
    c[0] = prev;
    for (int i = 1; i < n; ++i) {
        prev = 6.f * c[(long)i * s] + z * prev;
        c[(long)i * s] = prev;
    }
    // anti-causal init from the last two causal values, then the backward pass
    float next = (z * c[(long)(n - 2) * s] + prev) * z / (z * z - 1.f);
    c[(long)(n - 1) * s] = next;
    for (int i = n - 2; i >= 0; --i) {
        next = z * (next - c[(long)i * s]);
        c[(long)i * s] = next;
    }
}

// Lines along D (axis 0) or H (axis 1): one lane per line, consecutive lanes on consecutive x (coalesced).
__global__ void k_bspline_prefilter_strided(float *__restrict__ x, int C, int D, int H, int W, int axis) {
    const long lines = axis == 0 ? (long)C * H * W : (long)C * D * W;
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= lines) return;
    long base, s;
    int n;
    if (axis == 0) {
        const long hw = (long)H * W;
        base = (l / hw) * D * hw + l % hw;
        s = hw;
        n = D;
    } else {
        base = (l / W) * H * W + l % W;  // (c, z) plane, then x
        s = W;
        n = H;
    }
    bspline3_line(x + base, n, s);
}

// Lines along W (contiguous rows): a block stages `rows` consecutive rows in LDS with an odd row pitch (lane t filters
// row t: bank-conflict free), then writes them back coalesced.
__global__ void k_bspline_prefilter_rows(float *__restrict__ x, long nrows, int W, int pitch, int rows) {
    extern __shared__ float lds[];
    const long r0 = (long)blockIdx.x * rows;
    const int nr = (int)(nrows - r0 < rows ? nrows - r0 : rows);
    const long n = (long)nr * W;
    float *g = x + r0 * W;
    for (long i = threadIdx.x; i < n; i += blockDim.x) lds[(i / W) * pitch + i % W] = g[i];
    __syncthreads();
    if ((int)threadIdx.x < nr) bspline3_line(lds + threadIdx.x * pitch, W, 1);
    __syncthreads();
    for (long i = threadIdx.x; i < n; i += blockDim.x) g[i] = lds[(i / W) * pitch + i % W];
}

struct Affine12 {
    double a[12];  // A row-major (3x3), then the offset (3)
};

// scipy's mirror extension of a tap index (... c b | a b c ... | ... b a), period 2n - 2
__device__ __forceinline__ int mirror_index(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * n - 2;
    int m = (i < 0 ? -i : i) % period;
    return m >= n ? period - m : m;
}

// Output voxel of this lane: 8 (x) x 8 (y) x 4 (z) voxels per 256-lane block.
__device__ __forceinline__ bool warp_voxel(int fd, int fh, int fw, int &oz, int &oy, int &ox) {
    ox = blockIdx.x * 8 + (threadIdx.x & 7);
    oy = blockIdx.y * 8 + ((threadIdx.x >> 3) & 7);
    oz = blockIdx.z * 4 + (threadIdx.x >> 6);
    return ox < fw && oy < fh && oz < fd;
}

// Input coordinate of output voxel o, relative to the patch centre in fp64; false when outside [0, n-1] on any axis.
__device__ __forceinline__ bool warp_coord(const Affine12 &T, int oz, int oy, int ox, int fd, int fh, int fw, int D,
                                           int H, int W, double (&p)[3]) {
    const double q0 = oz - 0.5 * (fd - 1), q1 = oy - 0.5 * (fh - 1), q2 = ox - 0.5 * (fw - 1);
    const int n[3] = {D, H, W};
    bool inside = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        p[d] = T.a[3 * d] * q0 + T.a[3 * d + 1] * q1 + T.a[3 * d + 2] * q2 + T.a[9 + d];
        inside = inside && p[d] >= 0.0 && p[d] <= (double)(n[d] - 1);
    }
    return inside;
}

__device__ __forceinline__ long flipped_index(int oz, int oy, int ox, int fd, int fh, int fw, int flip_mask) {
    const int sz = (flip_mask & 1) ? fd - 1 - oz : oz;
    const int sy = (flip_mask & 2) ? fh - 1 - oy : oy;
    const int sx = (flip_mask & 4) ? fw - 1 - ox : ox;
    return ((long)sz * fh + sy) * fw + sx;
}

__device__ __forceinline__ void cubic_weights(float t, float (&w)[4]) {
    const float t2 = t * t, t3 = t2 * t, u = 1.f - t;
    w[0] = u * u * u * (1.f / 6.f);
    w[1] = (4.f - 6.f * t2 + 3.f * t3) * (1.f / 6.f);
    w[2] = (1.f + 3.f * t + 3.f * t2 - 3.f * t3) * (1.f / 6.f);
    w[3] = t3 * (1.f / 6.f);
}

// out[c][flip(o)] = sum of the 4x4x4 taps of coef[c] at p(o) (cval outside the domain).  Coordinate, domain test,
// weights and tap offsets once per voxel; the channel loop reuses them.
__global__ void __launch_bounds__(256) k_spatial_warp_data(const float *__restrict__ coef, float *__restrict__ out,
                                                           int C, int D, int H, int W, int fd, int fh, int fw,
                                                           Affine12 T, int flip_mask, float cval) {
    int oz, oy, ox;
    if (!warp_voxel(fd, fh, fw, oz, oy, ox)) return;
    const long ovol = (long)fd * fh * fw, ivol = (long)D * H * W;
    const long o = flipped_index(oz, oy, ox, fd, fh, fw, flip_mask);
    double p[3];
    if (!warp_coord(T, oz, oy, ox, fd, fh, fw, D, H, W, p)) {
        for (int c = 0; c < C; ++c) out[c * ovol + o] = cval;
        return;
    }
    const int n[3] = {D, H, W};
    float w[3][4];
    int idx[3][4];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double f = floor(p[d]);
        cubic_weights((float)(p[d] - f), w[d]);
#pragma unroll
        for (int k = 0; k < 4; ++k) idx[d][k] = mirror_index((int)f - 1 + k, n[d]);
    }
    int rzy[16];  // row offsets of the 4x4 (z, y) taps; D*H*W < 2^31 (checked at the entry)
#pragma unroll
    for (int k = 0; k < 16; ++k) rzy[k] = (idx[0][k >> 2] * H + idx[1][k & 3]) * W;
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        const float *src = coef + c * ivol;
        float acc = 0.f;
#pragma unroll 1
        for (int a = 0; a < 4; ++a) {  // not unrolled: 64 hoisted tap addresses would cost 2 waves/SIMD
            float accy = 0.f;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float *row = src + rzy[4 * a + b];
                const float v = w[2][0] * row[idx[2][0]] + w[2][1] * row[idx[2][1]] + w[2][2] * row[idx[2][2]] +
                                w[2][3] * row[idx[2][3]];
                accy += w[1][b] * v;
            }
            acc += w[0][a] * accy;
        }
        out[c * ovol + o] = acc;
    }
}

// out[c][flip(o)] = the largest label L among the 8 linear taps whose indicator sum reaches 0.5, else 0 (also outside
// the domain, where every indicator is the cval -1); then L == rep_from becomes rep_to when do_rep.
__global__ void __launch_bounds__(256) k_spatial_warp_seg(const float *__restrict__ seg, float *__restrict__ out, int C,
                                                          int D, int H, int W, int fd, int fh, int fw, Affine12 T,
                                                          int flip_mask, int do_rep, float rep_from, float rep_to) {
    int oz, oy, ox;
    if (!warp_voxel(fd, fh, fw, oz, oy, ox)) return;
    const long ovol = (long)fd * fh * fw, ivol = (long)D * H * W;
    const long o = flipped_index(oz, oy, ox, fd, fh, fw, flip_mask);
    double p[3];
    const bool inside = warp_coord(T, oz, oy, ox, fd, fh, fw, D, H, W, p);
    const int n[3] = {D, H, W};
    float w[3][2];
    int idx[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double f = inside ? floor(p[d]) : 0.0;
        const float t = inside ? (float)(p[d] - f) : 0.f;
        w[d][0] = 1.f - t;
        w[d][1] = t;
        idx[d][0] = (int)f;
        idx[d][1] = mirror_index((int)f + 1, n[d]);
    }
    float wt[8];
    long off[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        wt[k] = w[0][k >> 2] * w[1][(k >> 1) & 1] * w[2][k & 1];
        off[k] = ((long)idx[0][k >> 2] * H + idx[1][(k >> 1) & 1]) * W + idx[2][k & 1];
    }
    for (int c = 0; c < C; ++c) {
        float res = 0.f;
        if (inside) {
            const float *src = seg + c * ivol;
            float lab[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) lab[k] = src[off[k]];
            bool found = false;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float ind = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) ind += lab[j] == lab[k] ? wt[j] : 0.f;
                if (ind >= 0.5f && (!found || lab[k] > res)) {
                    res = lab[k];
                    found = true;
                }
            }
        }
        if (do_rep && res == rep_from) res = rep_to;
        out[c * ovol + o] = res;
    }
}

// ------------------------------------------------------------------------------------------------ in-plane (dummy 2-D)
// Convert3DTo2DTransform around the SpatialTransform (nnUNetTrainer.py:695-717): [C][D][H][W] is [C*D][H][W] and one
// in-plane map p(oy, ox) = A (o - (f-1)/2) + off moves every slice of every channel.  A lane owns one (oy, ox) of a
// 16 x 16 tile and walks kPlanesPerBlock consecutive planes (c, z); grid.z deals the planes.
struct Affine6 {
    double a[6];  // A row-major (2x2), then the offset (2)
};

constexpr int kPlanesPerBlock = 8;

__device__ __forceinline__ bool warp2d_pixel(int fh, int fw, int &oy, int &ox) {
    ox = blockIdx.x * 16 + (threadIdx.x & 15);
    oy = blockIdx.y * 16 + (threadIdx.x >> 4);
    return ox < fw && oy < fh;
}

__device__ __forceinline__ bool warp2d_coord(const Affine6 &T, int oy, int ox, int fh, int fw, int H, int W,
                                             double (&p)[2]) {
    const double q0 = oy - 0.5 * (fh - 1), q1 = ox - 0.5 * (fw - 1);
    p[0] = T.a[0] * q0 + T.a[1] * q1 + T.a[4];
    p[1] = T.a[2] * q0 + T.a[3] * q1 + T.a[5];
    return p[0] >= 0.0 && p[0] <= (double)(H - 1) && p[1] >= 0.0 && p[1] <= (double)(W - 1);
}

// Walk of the planes [p0, p1) of one block: `in` is the plane read, `out` the plane stored.  Bit 0 of flip_mask mirrors
// the slice index inside its channel (MirrorTransform runs after Convert2DTo3DTransform).  Wave-uniform.
struct PlaneWalk {
    long c, p1;
    int z, D, flip;
    __device__ __forceinline__ PlaneWalk(long planes, int D_, int flip_mask) : D(D_), flip(flip_mask & 1) {
        const long p0 = (long)blockIdx.z * kPlanesPerBlock;
        p1 = p0 + kPlanesPerBlock < planes ? p0 + kPlanesPerBlock : planes;
        c = p0 / D;
        z = (int)(p0 - c * D);
    }
    __device__ __forceinline__ bool more() const { return c * D + z < p1; }
    __device__ __forceinline__ long in() const { return c * D + z; }
    __device__ __forceinline__ long out() const { return c * D + (flip ? D - 1 - z : z); }
    __device__ __forceinline__ void next() {
        if (++z == D) {
            z = 0;
            ++c;
        }
    }
};

// One tap: a wave-uniform plane base plus a 32-bit byte offset (H*W < 2^30, checked at the entry).
__device__ __forceinline__ float tap(const float *plane, unsigned boff) {
    return *reinterpret_cast<const float *>(reinterpret_cast<const char *>(plane) + boff);
}

// out[c][flip(z, oy, ox)] = sum of the 4x4 taps of slice (c, z) of coef at p(oy, ox) (cval outside the domain).
// Coordinate, domain test, weights and the 16 tap offsets once per lane; the plane walk reuses them.
__global__ void __launch_bounds__(256) k_spatial_warp2d_data(const float *__restrict__ coef, float *__restrict__ out,
                                                             long planes, int D, int H, int W, int fh, int fw,
                                                             Affine6 T, int flip_mask, float cval) {
    int oy, ox;
    if (!warp2d_pixel(fh, fw, oy, ox)) return;
    const long oarea = (long)fh * fw, iarea = (long)H * W;
    const int sy = (flip_mask & 2) ? fh - 1 - oy : oy, sx = (flip_mask & 4) ? fw - 1 - ox : ox;
    const long o = (long)sy * fw + sx;
    PlaneWalk pw(planes, D, flip_mask);
    double p[2];
    if (!warp2d_coord(T, oy, ox, fh, fw, H, W, p)) {
        for (; pw.more(); pw.next()) out[pw.out() * oarea + o] = cval;
        return;
    }
    const int n[2] = {H, W};
    float w[2][4];
    int idx[2][4];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const double f = floor(p[d]);
        cubic_weights((float)(p[d] - f), w[d]);
#pragma unroll
        for (int k = 0; k < 4; ++k) idx[d][k] = mirror_index((int)f - 1 + k, n[d]);
    }
    unsigned off[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) off[k] = 4u * (unsigned)(idx[0][k >> 2] * W + idx[1][k & 3]);
#pragma clang loop vectorize(disable) unroll(disable)
    for (; pw.more(); pw.next()) {
        const float *src = coef + pw.in() * iarea;
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float v = w[1][0] * tap(src, off[4 * a]) + w[1][1] * tap(src, off[4 * a + 1]) +
                            w[1][2] * tap(src, off[4 * a + 2]) + w[1][3] * tap(src, off[4 * a + 3]);
            acc += w[0][a] * v;
        }
        out[pw.out() * oarea + o] = acc;
    }
}

// The same walk with the 4 bilinear taps and k_spatial_warp_seg's winner rule: the largest label whose indicator sum
// reaches 0.5, 0 otherwise and outside; then L == rep_from becomes rep_to when do_rep.
__global__ void __launch_bounds__(256) k_spatial_warp2d_seg(const float *__restrict__ seg, float *__restrict__ out,
                                                            long planes, int D, int H, int W, int fh, int fw, Affine6 T,
                                                            int flip_mask, int do_rep, float rep_from, float rep_to) {
    int oy, ox;
    if (!warp2d_pixel(fh, fw, oy, ox)) return;
    const long oarea = (long)fh * fw, iarea = (long)H * W;
    const int sy = (flip_mask & 2) ? fh - 1 - oy : oy, sx = (flip_mask & 4) ? fw - 1 - ox : ox;
    const long o = (long)sy * fw + sx;
    PlaneWalk pw(planes, D, flip_mask);
    double p[2];
    if (!warp2d_coord(T, oy, ox, fh, fw, H, W, p)) {
        const float res = (do_rep && 0.f == rep_from) ? rep_to : 0.f;
        for (; pw.more(); pw.next()) out[pw.out() * oarea + o] = res;
        return;
    }
    const int n[2] = {H, W};
    float w[2][2];
    int idx[2][2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const double f = floor(p[d]);
        const float t = (float)(p[d] - f);
        w[d][0] = 1.f - t;
        w[d][1] = t;
        idx[d][0] = (int)f;
        idx[d][1] = mirror_index((int)f + 1, n[d]);
    }
    float wt[4];
    unsigned off[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        wt[k] = w[0][k >> 1] * w[1][k & 1];
        off[k] = 4u * (unsigned)(idx[0][k >> 1] * W + idx[1][k & 1]);
    }
#pragma clang loop vectorize(disable)
    for (; pw.more(); pw.next()) {
        const float *src = seg + pw.in() * iarea;
        float lab[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) lab[k] = tap(src, off[k]);
        float res = 0.f;
        bool found = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float ind = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) ind += lab[j] == lab[k] ? wt[j] : 0.f;
            if (ind >= 0.5f && (!found || lab[k] > res)) {
                res = lab[k];
                found = true;
            }
        }
        if (do_rep && res == rep_from) res = rep_to;
        out[pw.out() * oarea + o] = res;
    }
}

}  // namespace mvd

using namespace mvd;

static bool spatial_shape_ok(int C, int D, int H, int W, int fd, int fh, int fw) {
    const int lim = 1 << 30;
    if (C <= 0 || D <= 0 || H <= 0 || W <= 0 || fd <= 0 || fh <= 0 || fw <= 0) return false;
    if (D >= lim || H >= lim || W >= lim || fd >= lim || fh >= lim || fw >= lim) return false;
    if ((long)D * H * W >= (1L << 31)) return false;  // 32-bit tap offsets within one channel
    // grid.y / grid.z limits of the 8x8x4 warp tiling
    return (fh + 7) / 8 < 65536 && (fd + 3) / 4 < 65536;
}

static bool affine_ok(const double *a) {
    for (int i = 0; i < 12; ++i)
        if (!(a[i] == a[i]) || a[i] > 1e9 || a[i] < -1e9) return false;  // NaN / inf / absurd
    return true;
}

static Affine12 load_affine(const double *a) {
    Affine12 t;
    for (int i = 0; i < 12; ++i) t.a[i] = a[i];
    return t;
}

static dim3 warp_grid(int fd, int fh, int fw) { return dim3((fw + 7) / 8, (fh + 7) / 8, (fd + 3) / 4); }

static bool spatial2d_shape_ok(int C, int D, int H, int W, int fh, int fw) {
    const int lim = 1 << 30;
    if (C <= 0 || D <= 0 || H <= 0 || W <= 0 || fh <= 0 || fw <= 0) return false;
    if (D >= lim || H >= lim || W >= lim || fh >= lim || fw >= lim) return false;
    if ((long)H * W >= (1L << 30)) return false;  // 32-bit tap byte offsets within one plane
    if ((long)C * D >= (long)kPlanesPerBlock * 65535) return false;  // grid.z
    return (fh + 15) / 16 < 65536;                                   // grid.y
}

static bool affine6_ok(const double *a) {
    for (int i = 0; i < 6; ++i)
        if (!(a[i] == a[i]) || a[i] > 1e9 || a[i] < -1e9) return false;
    return true;
}

static Affine6 load_affine6(const double *a) {
    Affine6 t;
    for (int i = 0; i < 6; ++i) t.a[i] = a[i];
    return t;
}

static dim3 warp2d_grid(long planes, int fh, int fw) {
    return dim3((fw + 15) / 16, (fh + 15) / 16, (unsigned)cdiv(planes, (long)kPlanesPerBlock));
}

extern "C" {

int mvd_feed_bspline_prefilter_f32(float *x, int C, int D, int H, int W, int axis_mask, void *stream) {
    MVD_REQUIRE(x, "feed_bspline_prefilter_f32: null pointer");
    MVD_REQUIRE(spatial_shape_ok(C, D, H, W, 1, 1, 1), "feed_bspline_prefilter_f32: bad shape");
    MVD_REQUIRE(axis_mask >= 0 && axis_mask < 8, "feed_bspline_prefilter_f32: axis_mask is a 3-bit axis mask");
    hipStream_t s = as_stream(stream);
    for (int axis = 0; axis < 2; ++axis) {
        if (!(axis_mask & (1 << axis)) || (axis == 0 ? D : H) < 2) continue;
        const long lines = axis == 0 ? (long)C * H * W : (long)C * D * W;
        hipLaunchKernelGGL(k_bspline_prefilter_strided, dim3((unsigned)cdiv(lines, 256)), dim3(256), 0, s, x, C, D, H,
                           W, axis);
        int e = check_launch("feed_bspline_prefilter_f32");
        if (e) return e;
    }
    if ((axis_mask & 4) && W >= 2) {
        const int pitch = W | 1;
        const long max_lds = 64 * 1024;
        MVD_REQUIRE((long)pitch * 4 <= max_lds, "feed_bspline_prefilter_f32: W too large for the LDS row stage");
        int rows = (int)(max_lds / (4L * pitch));
        if (rows > 64) rows = 64;
        const long nrows = (long)C * D * H;
        hipLaunchKernelGGL(k_bspline_prefilter_rows, dim3((unsigned)cdiv(nrows, rows)), dim3(64),
                           (size_t)rows * pitch * sizeof(float), s, x, nrows, W, pitch, rows);
        return check_launch("feed_bspline_prefilter_f32");
    }
    return 0;
}

int mvd_feed_warp_data_f32(const float *coef, float *out, int C, int D, int H, int W, int fd, int fh, int fw,
                           const double *affine12, int flip_mask, float cval, void *stream) {
    MVD_REQUIRE(coef && out && affine12, "feed_warp_data_f32: null pointer");
    MVD_REQUIRE(spatial_shape_ok(C, D, H, W, fd, fh, fw), "feed_warp_data_f32: bad shape");
    MVD_REQUIRE(flip_mask >= 0 && flip_mask < 8, "feed_warp_data_f32: flip_mask is a 3-bit axis mask");
    MVD_REQUIRE(affine_ok(affine12), "feed_warp_data_f32: affine12 must be finite");
    hipLaunchKernelGGL(k_spatial_warp_data, warp_grid(fd, fh, fw), dim3(256), 0, as_stream(stream), coef, out, C, D, H,
                       W, fd, fh, fw, load_affine(affine12), flip_mask, cval);
    return check_launch("feed_warp_data_f32");
}

int mvd_feed_warp_seg(const float *seg, float *out, int C, int D, int H, int W, int fd, int fh, int fw,
                      const double *affine12, int flip_mask, int replace, int replace_from, int replace_to,
                      void *stream) {
    MVD_REQUIRE(seg && out && affine12, "feed_warp_seg: null pointer");
    MVD_REQUIRE(spatial_shape_ok(C, D, H, W, fd, fh, fw), "feed_warp_seg: bad shape");
    MVD_REQUIRE(flip_mask >= 0 && flip_mask < 8, "feed_warp_seg: flip_mask is a 3-bit axis mask");
    MVD_REQUIRE(affine_ok(affine12), "feed_warp_seg: affine12 must be finite");
    hipLaunchKernelGGL(k_spatial_warp_seg, warp_grid(fd, fh, fw), dim3(256), 0, as_stream(stream), seg, out, C, D, H, W,
                       fd, fh, fw, load_affine(affine12), flip_mask, replace ? 1 : 0, (float)replace_from,
                       (float)replace_to);
    return check_launch("feed_warp_seg");
}

int mvd_feed_warp2d_data_f32(const float *coef, float *out, int C, int D, int H, int W, int fh, int fw,
                             const double *affine6, int flip_mask, float cval, void *stream) {
    MVD_REQUIRE(coef && out && affine6, "feed_warp2d_data_f32: null pointer");
    MVD_REQUIRE(spatial2d_shape_ok(C, D, H, W, fh, fw), "feed_warp2d_data_f32: bad shape");
    MVD_REQUIRE(flip_mask >= 0 && flip_mask < 8, "feed_warp2d_data_f32: flip_mask is a 3-bit axis mask");
    MVD_REQUIRE(affine6_ok(affine6), "feed_warp2d_data_f32: affine6 must be finite");
    const long planes = (long)C * D;
    hipLaunchKernelGGL(k_spatial_warp2d_data, warp2d_grid(planes, fh, fw), dim3(256), 0, as_stream(stream), coef, out,
                       planes, D, H, W, fh, fw, load_affine6(affine6), flip_mask, cval);
    return check_launch("feed_warp2d_data_f32");
}

int mvd_feed_warp2d_seg(const float *seg, float *out, int C, int D, int H, int W, int fh, int fw, const double *affine6,
                        int flip_mask, int replace, int replace_from, int replace_to, void *stream) {
    MVD_REQUIRE(seg && out && affine6, "feed_warp2d_seg: null pointer");
    MVD_REQUIRE(spatial2d_shape_ok(C, D, H, W, fh, fw), "feed_warp2d_seg: bad shape");
    MVD_REQUIRE(flip_mask >= 0 && flip_mask < 8, "feed_warp2d_seg: flip_mask is a 3-bit axis mask");
    MVD_REQUIRE(affine6_ok(affine6), "feed_warp2d_seg: affine6 must be finite");
    const long planes = (long)C * D;
    hipLaunchKernelGGL(k_spatial_warp2d_seg, warp2d_grid(planes, fh, fw), dim3(256), 0, as_stream(stream), seg, out,
                       planes, D, H, W, fh, fw, load_affine6(affine6), flip_mask, replace ? 1 : 0, (float)replace_from,
                       (float)replace_to);
    return check_launch("feed_warp2d_seg");
}
}
