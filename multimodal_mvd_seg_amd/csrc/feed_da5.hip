// On-device kernels of the DA5 augmentation recipe of the training feed: the transforms nnUNetTrainerDA5 adds
// to the default pipeline.  The numeric cores are pinned to numpy / scipy:
//   k_median_filter     scipy.ndimage.median_filter(size = s, mode 'reflect'), s = 2..7: an exact selection.  An 8^3 output
//                       tile and its halo sit in LDS as order-preserving uint32 keys; each voxel finds the key of rank
//                       s^3 / 2 by a bitwise descent (32 counting passes over its window), no sort, no per-lane window copy
//   k_sharpen           scipy.signal.convolve(x, strength L + delta, 'same') (7-point stencil, zero border), clipped to the
//                       channel's own range
//   k_local_gauss       the separable Gaussian field of the two LocalTransforms (additive gradient, local gamma); the
//                       per-axis exponentials are tabulated once per block in LDS, in fp64
//   k_rect_sum / _fill  BlankRectangleTransform with the box mean: fp64 sum in a fixed two-level order, rounded once
//   k_signed_permute*   flip(transpose(x, perm), mask): Rot90Transform, TransposeAxesTransform and the mirror; through a
//                       32 x 32 LDS tile when perm moves the W axis, so loads and stores both run along contiguous memory
//   k_blur_axis_wide    k_gaussian_blur_axis of feed_intensity.hip with a radius of up to 6 (sigma <= 1.5)
//   k_da5_apply         additive brightness, contrast without the clip (preserve_range=False)
// Planar fp32 [C][D][H][W]; per-channel parameters travel by value in the kernel arguments.  No float atomics: every
// result is bit-identical from run to run.  NaN inputs are unsupported (the median's key order puts them at the ends).
#include "common.h"

namespace mvd {

constexpr int kMaxCh = 16;

struct ChanF {
    float v[kMaxCh];
};
struct ChanD {
    double v[kMaxCh];
};
struct ChanI {
    int v[kMaxCh];
};

__device__ __forceinline__ bool chan_on(int mask, int c) { return (mask >> c) & 1; }

// scipy 'reflect' (d c b a | a b c d | d c b a), repeated on lines shorter than the overhang
__device__ __forceinline__ int reflect_index(int i, int n) {
    const int p = 2 * n;
    int m = i % p;
    m = m < 0 ? m + p : m;
    return m < n ? m : p - 1 - m;
}

// ------------------------------------------------------------------------------------------------ median
constexpr int kMedT = 8;                 // output tile edge
constexpr int kMedE = kMedT + 6;         // tile + the halo of the widest window (s = 7)
constexpr int kMedThreads = 256;

// fp32 -> uint32 with the order of the floats (-0.0 sorts just below +0.0; they compare equal as values)
__device__ __forceinline__ unsigned key_of(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// The window at index i covers i - S/2 .. i + (S-1) - S/2.  The answer is the largest T with #(keys < T) <= rank, built
// bit by bit from the top.  The z loop is kept rolled so that the window is re-read from LDS in every pass instead of
// being hoisted into S^3 registers.
template <int S>
__device__ __forceinline__ void median_tile(const float *__restrict__ xc, float *__restrict__ oc, int D, int H, int W,
                                            int z0, int y0, int x0, unsigned *keys) {
    constexpr int E = kMedT + S - 1;
    constexpr int R = (S * S * S) / 2;
    const int lo = S / 2;
    for (int i = threadIdx.x; i < E * E * E; i += kMedThreads) {
        const int ix = i % E, iy = (i / E) % E, iz = i / (E * E);
        const int gz = reflect_index(z0 - lo + iz, D), gy = reflect_index(y0 - lo + iy, H),
                  gx = reflect_index(x0 - lo + ix, W);
        keys[(iz * kMedE + iy) * kMedE + ix] = key_of(xc[((long)gz * H + gy) * W + gx]);
    }
    __syncthreads();
    for (int v = threadIdx.x; v < kMedT * kMedT * kMedT; v += kMedThreads) {
        const int lx = v & 7, ly = (v >> 3) & 7, lz = v >> 6;
        const int gz = z0 + lz, gy = y0 + ly, gx = x0 + lx;
        if (gz >= D || gy >= H || gx >= W) continue;
        const unsigned *base = keys + (lz * kMedE + ly) * kMedE + lx;
        unsigned t = 0u;
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            const unsigned cand = t | (1u << b);
            int cnt = 0;
#pragma unroll 1
            for (int dz = 0; dz < S; ++dz) {
                const unsigned *pz = base + dz * kMedE * kMedE;
#pragma unroll
                for (int dy = 0; dy < S; ++dy)
#pragma unroll
                    for (int dx = 0; dx < S; ++dx) cnt += pz[dy * kMedE + dx] < cand ? 1 : 0;
            }
            if (cnt <= R) t = cand;
        }
        oc[((long)gz * H + gy) * W + gx] = float_of(t);
    }
}

__global__ void __launch_bounds__(kMedThreads) k_median_filter(const float *__restrict__ x, float *__restrict__ out,
                                                               int D, int H, int W, int ntx, int nty, ChanI sizes) {
    __shared__ unsigned keys[kMedE * kMedE * kMedE];
    const int c = blockIdx.y;
    const int s = sizes.v[c];
    const long V = (long)D * H * W;
    const float *xc = x + c * V;
    float *oc = out + c * V;
    const int tx = blockIdx.x % ntx, ty = (blockIdx.x / ntx) % nty, tz = blockIdx.x / (ntx * nty);
    const int z0 = tz * kMedT, y0 = ty * kMedT, x0 = tx * kMedT;
    switch (s) {
        case 2: median_tile<2>(xc, oc, D, H, W, z0, y0, x0, keys); break;
        case 3: median_tile<3>(xc, oc, D, H, W, z0, y0, x0, keys); break;
        case 4: median_tile<4>(xc, oc, D, H, W, z0, y0, x0, keys); break;
        case 5: median_tile<5>(xc, oc, D, H, W, z0, y0, x0, keys); break;
        case 6: median_tile<6>(xc, oc, D, H, W, z0, y0, x0, keys); break;
        case 7: median_tile<7>(xc, oc, D, H, W, z0, y0, x0, keys); break;
        default:  // 0: the channel is copied
            for (int v = threadIdx.x; v < kMedT * kMedT * kMedT; v += kMedThreads) {
                const int gz = z0 + (v >> 6), gy = y0 + ((v >> 3) & 7), gx = x0 + (v & 7);
                if (gz < D && gy < H && gx < W) {
                    const long o = ((long)gz * H + gy) * W + gx;
                    oc[o] = xc[o];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------ sharpen
// ws[c] = clip((6 s + 1) x - s (sum of the face neighbours inside the volume), min, max) for the channels with s != 0
__global__ void __launch_bounds__(256) k_sharpen(const float *__restrict__ x, float *__restrict__ ws, int D, int H,
                                                 int W, ChanD strength, const double *__restrict__ stats) {
    const int c = blockIdx.y;
    const double sd = strength.v[c];
    if (sd == 0.0) return;
    const long V = (long)D * H * W;
    const float *xc = x + c * V;
    float *wc = ws + c * V;
    const float kc = (float)(6.0 * sd + 1.0), s = (float)sd;
    const float lo = (float)stats[4 * c + 2], hi = (float)stats[4 * c + 3];
    const long sy = W, sz = (long)H * W;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        const int ix = (int)(v % W), iy = (int)((v / W) % H), iz = (int)(v / sz);
        float nb = 0.f;
        if (iz > 0) nb += xc[v - sz];
        if (iy > 0) nb += xc[v - sy];
        if (ix > 0) nb += xc[v - 1];
        if (ix < W - 1) nb += xc[v + 1];
        if (iy < H - 1) nb += xc[v + sy];
        if (iz < D - 1) nb += xc[v + sz];
        const float r = kc * xc[v] - s * nb;
        wc[v] = r < lo ? lo : (r > hi ? hi : r);
    }
}

__global__ void __launch_bounds__(256) k_copy_selected(const float *__restrict__ ws, float *__restrict__ x, long V,
                                                       ChanD sel) {
    const int c = blockIdx.y;
    if (sel.v[c] == 0.0) return;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x)
        x[c * V + v] = ws[c * V + v];
}

// ------------------------------------------------------------------------------------------------ local Gaussian field
struct GaussArgs {
    double loc[kMaxCh][3];
    double scale[kMaxCh][3];
    float amount[kMaxCh];
};

// g = prod_d exp(-(i_d - loc_d)^2 / (2 scale_d^2)) / max g.  The maximum is separable (per axis at the grid index nearest
// to loc_d), so each axis table is normalised on its own: tab_d[i] = exp(-((i - loc)^2 - (i* - loc)^2) / (2 scale^2)).
__global__ void __launch_bounds__(256) k_local_gauss(float *__restrict__ x, int D, int H, int W, int chmask, int mode,
                                                     GaussArgs a, const double *__restrict__ stats) {
    extern __shared__ float tab[];  // [D] [H] [W]
    const int c = blockIdx.y;
    if (!chan_on(chmask, c)) return;
    for (int i = threadIdx.x; i < D + H + W; i += blockDim.x) {
        const int d = i < D ? 0 : (i < D + H ? 1 : 2);
        const int ii = d == 0 ? i : (d == 1 ? i - D : i - D - H);
        const int n = d == 0 ? D : (d == 1 ? H : W);
        const double loc = a.loc[c][d], sc = a.scale[c][d];
        double is = rint(loc);
        is = is < 0.0 ? 0.0 : (is > (double)(n - 1) ? (double)(n - 1) : is);
        const double q = ((double)ii - loc) * ((double)ii - loc) - (is - loc) * (is - loc);
        tab[i] = (float)exp(-q / (2.0 * sc * sc));
    }
    __syncthreads();
    const long V = (long)D * H * W;
    float *xc = x + c * V;
    const float amt = a.amount[c];
    float mn = 0.f, r = 0.f;
    if (mode == 1) {
        mn = (float)stats[4 * c + 2];
        r = (float)(stats[4 * c + 3] - stats[4 * c + 2]);
    }
    const float inv = 1.f / fmaxf(r, 1e-8f);
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        const int ix = (int)(v % W), iy = (int)((v / W) % H), iz = (int)(v / ((long)H * W));
        const float g = tab[iz] * tab[D + iy] * tab[D + H + ix];
        const float xv = xc[v];
        if (mode == 0) {
            xc[v] = xv + amt * g;
        } else {
            float b = (xv - mn) * inv;
            b = b > 0.f ? b : 0.f;
            xc[v] = powf(b, 1.f + (amt - 1.f) * g) * r + mn;
        }
    }
}

// ------------------------------------------------------------------------------------------------ blank rectangle
constexpr int kRectBlocks = 64;

struct Box {
    int lb[3];
    int sz[3];
};

// part[b] = the fp64 sum of box elements b chunk .. (b + 1) chunk (row-major in the box), lanes strided, fixed order
__global__ void __launch_bounds__(256) k_rect_sum(const float *__restrict__ xc, int H, int W, Box bx,
                                                  double *__restrict__ part) {
    __shared__ double sm[16];
    const long n = (long)bx.sz[0] * bx.sz[1] * bx.sz[2];
    const long chunk = (n + kRectBlocks - 1) / kRectBlocks;
    const long beg = (long)blockIdx.x * chunk;
    const long end = beg + chunk < n ? beg + chunk : n;
    double s[1] = {0.0};
    for (long i = beg + threadIdx.x; i < end; i += blockDim.x) {
        const int ix = (int)(i % bx.sz[2]), iy = (int)((i / bx.sz[2]) % bx.sz[1]),
                  iz = (int)(i / ((long)bx.sz[2] * bx.sz[1]));
        s[0] += (double)xc[((long)(bx.lb[0] + iz) * H + (bx.lb[1] + iy)) * W + (bx.lb[2] + ix)];
    }
    block_sum<1>(s, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

__global__ void __launch_bounds__(256) k_rect_fill(float *__restrict__ xc, int H, int W, Box bx,
                                                   const double *__restrict__ part) {
    const long n = (long)bx.sz[0] * bx.sz[1] * bx.sz[2];
    double s = 0.0;
    for (int b = 0; b < kRectBlocks; ++b) s += part[b];
    const float mean = (float)(s / (double)n);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int ix = (int)(i % bx.sz[2]), iy = (int)((i / bx.sz[2]) % bx.sz[1]),
                  iz = (int)(i / ((long)bx.sz[2] * bx.sz[1]));
        xc[((long)(bx.lb[0] + iz) * H + (bx.lb[1] + iy)) * W + (bx.lb[2] + ix)] = mean;
    }
}

// ------------------------------------------------------------------------------------------------ signed permutation
// out[o] = in[j] with j[perm[k]] = (mask bit k ? n_k - 1 - o_k : o_k): flip(transpose(in, perm), mask).  The permuted axes
// have equal extents, so out has the shape n = (D, H, W) of in.
struct Perm {
    int p[3];
    int n[3];
    int mask;
};

__device__ __forceinline__ long perm_src(const Perm &q, int o0, int o1, int o2) {
    const int v0 = (q.mask & 1) ? q.n[0] - 1 - o0 : o0;
    const int v1 = (q.mask & 2) ? q.n[1] - 1 - o1 : o1;
    const int v2 = (q.mask & 4) ? q.n[2] - 1 - o2 : o2;
    const int j0 = q.p[0] == 0 ? v0 : (q.p[1] == 0 ? v1 : v2);
    const int j1 = q.p[0] == 1 ? v0 : (q.p[1] == 1 ? v1 : v2);
    const int j2 = q.p[0] == 2 ? v0 : (q.p[1] == 2 ? v1 : v2);
    return ((long)j0 * q.n[1] + j1) * q.n[2] + j2;
}

// perm[2] == 2: the lanes run along W on both sides
__global__ void __launch_bounds__(256) k_signed_permute_rows(const float *__restrict__ in, float *__restrict__ out,
                                                             long V, Perm q) {
    const int c = blockIdx.y;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        const int o2 = (int)(v % q.n[2]), o1 = (int)((v / q.n[2]) % q.n[1]), o0 = (int)(v / ((long)q.n[2] * q.n[1]));
        out[c * V + v] = in[c * V + perm_src(q, o0, o1, o2)];
    }
}

// perm[2] != 2: the input's W axis lands on output axis ka (perm[ka] == 2).  A block moves a 32 x 32 tile over (output
// axis ka, output axis 2) at one index of the third output axis km: rows are loaded with the lanes along the input's W
// and stored with the lanes along the output's W.  block (32, 8); grid (tiles along W, tiles along ka, n_km * C).
__global__ void __launch_bounds__(256) k_signed_permute_tiled(const float *__restrict__ in, float *__restrict__ out,
                                                              long V, Perm q, int ka, int nka, int nkm) {
    __shared__ float tile[32][33];
    const int c = blockIdx.z / nkm, m = blockIdx.z % nkm;
    const int a0 = blockIdx.x * 32, b0 = blockIdx.y * 32;  // a: output axis 2, b: output axis ka
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int a = a0 + r, b = b0 + threadIdx.x;
        if (a < q.n[2] && b < nka) tile[r][threadIdx.x] = in[c * V + perm_src(q, ka == 0 ? b : m, ka == 0 ? m : b, a)];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int a = a0 + threadIdx.x, b = b0 + r;
        if (a < q.n[2] && b < nka)
            out[c * V + ((long)(ka == 0 ? b : m) * q.n[1] + (ka == 0 ? m : b)) * q.n[2] + a] = tile[threadIdx.x][r];
    }
}

// ------------------------------------------------------------------------------------------------ wide blur
struct BlurWideArgs {
    int ch[kMaxCh];      // selected channels
    int rad[kMaxCh];     // radius per selected channel (<= 6)
    float w[kMaxCh][7];  // w[k] = weight of offset +-k, normalised in fp64
};

// k_gaussian_blur_axis (feed_intensity.hip) with the longer weight table: the same arithmetic in the same order
__global__ void __launch_bounds__(256) k_blur_axis_wide(const float *__restrict__ in, float *__restrict__ out, int D,
                                                        int H, int W, int axis, BlurWideArgs a, int in_sel,
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

// ------------------------------------------------------------------------------------------------ pointwise
enum { kDa5Add = 0, kDa5ContrastNoClip = 1 };

__global__ void __launch_bounds__(256) k_da5_apply(float *__restrict__ x, long V, int chmask, int op, ChanF prm,
                                                   const double *__restrict__ stats) {
    const int c = blockIdx.y;
    if (!chan_on(chmask, c)) return;
    float *xc = x + c * V;
    const float p = prm.v[c];
    const float a = op == kDa5ContrastNoClip ? (float)stats[4 * c] : 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (long)gridDim.x * blockDim.x) {
        const float v = xc[i];
        xc[i] = op == kDa5Add ? v + p : (v - a) * p + a;
    }
}

}  // namespace mvd

using namespace mvd;

static unsigned stride_grid(long n, long cap) {
    long b = cdiv(n, 256);
    if (b > cap) b = cap;
    return (unsigned)(b < 1 ? 1 : b);
}

static bool shape_ok(int C, int D, int H, int W) {
    return C > 0 && C <= kMaxCh && D > 0 && H > 0 && W > 0 && D < (1 << 20) && H < (1 << 20) && W < (1 << 20) &&
           (long)D * H * W < (1L << 40);
}

extern "C" {

int mvd_feed_median_filter_f32(const float *x, float *out, int C, int D, int H, int W, const int *sizes, void *stream) {
    MVD_REQUIRE(x && out && sizes && x != out, "feed_median_filter_f32: null pointer, or x and out are the same buffer");
    MVD_REQUIRE(shape_ok(C, D, H, W), "feed_median_filter_f32: bad shape (1 <= C <= 16)");
    ChanI s = {};
    for (int c = 0; c < C; ++c) {
        MVD_REQUIRE(sizes[c] == 0 || (sizes[c] >= 2 && sizes[c] <= 7),
                    "feed_median_filter_f32: the filter size of channel %d is %d; sizes are 2..7, or 0 to copy the channel",
                    c, sizes[c]);
        s.v[c] = sizes[c];
    }
    const long ntx = cdiv(W, kMedT), nty = cdiv(H, kMedT), ntz = cdiv(D, kMedT);
    MVD_REQUIRE(ntx * nty * ntz < (1L << 31), "feed_median_filter_f32: volume too large");
    hipLaunchKernelGGL(k_median_filter, dim3((unsigned)(ntx * nty * ntz), C), dim3(kMedThreads), 0, as_stream(stream), x,
                       out, D, H, W, (int)ntx, (int)nty, s);
    return check_launch("feed_median_filter_f32");
}

int mvd_feed_sharpen_f32(float *x, float *ws, int C, int D, int H, int W, const double *strength, const double *stats,
                         void *stream) {
    MVD_REQUIRE(x && ws && strength && stats, "feed_sharpen_f32: null pointer");
    MVD_REQUIRE(shape_ok(C, D, H, W), "feed_sharpen_f32: bad shape (1 <= C <= 16)");
    ChanD s = {};
    bool any = false;
    for (int c = 0; c < C; ++c) {
        s.v[c] = strength[c];
        any = any || strength[c] != 0.0;
    }
    if (!any) return 0;
    const long V = (long)D * H * W;
    hipStream_t st = as_stream(stream);
    const dim3 grid(stride_grid(V, 2048), C);
    hipLaunchKernelGGL(k_sharpen, grid, dim3(256), 0, st, x, ws, D, H, W, s, stats);
    int e = check_launch("feed_sharpen_f32");
    if (e) return e;
    hipLaunchKernelGGL(k_copy_selected, grid, dim3(256), 0, st, ws, x, V, s);
    return check_launch("feed_sharpen_f32");
}

int mvd_feed_local_gauss_f32(float *x, int C, int D, int H, int W, int chmask, int mode, const double *loc,
                             const double *scale, const float *amount, const double *stats, void *stream) {
    MVD_REQUIRE(x && loc && scale && amount, "feed_local_gauss_f32: null pointer");
    MVD_REQUIRE(shape_ok(C, D, H, W) && chmask >= 0 && chmask < (1 << C), "feed_local_gauss_f32: bad shape (1 <= C <= 16)");
    MVD_REQUIRE(mode == 0 || mode == 1, "feed_local_gauss_f32: mode is 0 (additive gradient) or 1 (local gamma)");
    MVD_REQUIRE(mode == 0 || stats, "feed_local_gauss_f32: the local gamma needs the channel statistics");
    MVD_REQUIRE((long)D + H + W <= 12288, "feed_local_gauss_f32: D + H + W <= 12288 (the axis tables live in LDS)");
    GaussArgs a = {};
    for (int c = 0; c < C; ++c) {
        for (int d = 0; d < 3; ++d) {
            a.loc[c][d] = loc[3 * c + d];
            a.scale[c][d] = scale[3 * c + d];
            MVD_REQUIRE(!((chmask >> c) & 1) || scale[3 * c + d] > 0.0, "feed_local_gauss_f32: scale > 0");
        }
        a.amount[c] = amount[c];
    }
    if (chmask == 0) return 0;
    const long V = (long)D * H * W;
    // each block tabulates D + H + W exponentials: give it at least 4096 voxels
    hipLaunchKernelGGL(k_local_gauss, dim3(stride_grid(cdiv(V, 16), 1024), C), dim3(256), (size_t)(D + H + W) * 4,
                       as_stream(stream), x, D, H, W, chmask, mode, a, stats);
    return check_launch("feed_local_gauss_f32");
}

int mvd_feed_blank_rectangle_f32(float *x, int C, int D, int H, int W, int c, const int *lb, const int *size, double *ws,
                                 void *stream) {
    MVD_REQUIRE(x && lb && size && ws, "feed_blank_rectangle_f32: null pointer");
    MVD_REQUIRE(shape_ok(C, D, H, W) && c >= 0 && c < C, "feed_blank_rectangle_f32: bad shape (1 <= C <= 16, 0 <= c < C)");
    const int n[3] = {D, H, W};
    Box bx;
    for (int d = 0; d < 3; ++d) {
        MVD_REQUIRE(size[d] >= 1 && lb[d] >= 0 && (long)lb[d] + size[d] <= n[d],
                    "feed_blank_rectangle_f32: the box must lie inside the patch (axis %d: lb %d, size %d, extent %d)", d,
                    lb[d], size[d], n[d]);
        bx.lb[d] = lb[d];
        bx.sz[d] = size[d];
    }
    float *xc = x + (long)c * D * H * W;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_rect_sum, dim3(kRectBlocks), dim3(256), 0, st, xc, H, W, bx, ws);
    int e = check_launch("feed_blank_rectangle_f32");
    if (e) return e;
    const long nb = (long)size[0] * size[1] * size[2];
    hipLaunchKernelGGL(k_rect_fill, dim3(stride_grid(nb, 1024)), dim3(256), 0, st, xc, H, W, bx, ws);
    return check_launch("feed_blank_rectangle_f32");
}

int mvd_feed_signed_permute_f32(const float *in, float *out, int C, int D, int H, int W, const int *perm, int flip_mask,
                                void *stream) {
    MVD_REQUIRE(in && out && perm && in != out, "feed_signed_permute_f32: null pointer, or in and out are the same buffer");
    MVD_REQUIRE(C > 0 && C <= 4096 && shape_ok(1, D, H, W), "feed_signed_permute_f32: bad shape");
    MVD_REQUIRE(flip_mask >= 0 && flip_mask < 8, "feed_signed_permute_f32: flip_mask is a 3-bit axis mask");
    int seen = 0;
    for (int k = 0; k < 3; ++k) {
        MVD_REQUIRE(perm[k] >= 0 && perm[k] < 3, "feed_signed_permute_f32: perm is a permutation of (0, 1, 2)");
        seen |= 1 << perm[k];
    }
    MVD_REQUIRE(seen == 7, "feed_signed_permute_f32: perm is a permutation of (0, 1, 2)");
    Perm q;
    q.n[0] = D;
    q.n[1] = H;
    q.n[2] = W;
    q.mask = flip_mask;
    for (int k = 0; k < 3; ++k) {
        q.p[k] = perm[k];
        MVD_REQUIRE(q.n[perm[k]] == q.n[k],
                    "feed_signed_permute_f32: permuted axes must have equal length (axis %d has %d, axis %d has %d)", k,
                    q.n[k], perm[k], q.n[perm[k]]);
    }
    const long V = (long)D * H * W;
    hipStream_t st = as_stream(stream);
    if (perm[2] == 2) {
        MVD_REQUIRE(C <= 65535, "feed_signed_permute_f32: too many channels");
        hipLaunchKernelGGL(k_signed_permute_rows, dim3(stride_grid(V, 2048), C), dim3(256), 0, st, in, out, V, q);
    } else {
        const int ka = perm[0] == 2 ? 0 : 1, km = 1 - ka;
        MVD_REQUIRE((long)q.n[km] * C <= 65535 && cdiv(q.n[ka], 32) <= 65535,
                    "feed_signed_permute_f32: too many planes for one launch");
        hipLaunchKernelGGL(k_signed_permute_tiled, dim3((unsigned)cdiv(W, 32), (unsigned)cdiv(q.n[ka], 32), q.n[km] * C),
                           dim3(32, 8), 0, st, in, out, V, q, ka, q.n[ka], q.n[km]);
    }
    return check_launch("feed_signed_permute_f32");
}

int mvd_feed_gaussian_blur_wide_f32(float *x, float *ws, int C, int D, int H, int W, const double *sigma, void *stream) {
    MVD_REQUIRE(x && ws && sigma, "feed_gaussian_blur_wide_f32: null pointer");
    MVD_REQUIRE(shape_ok(C, D, H, W), "feed_gaussian_blur_wide_f32: bad shape (1 <= C <= 16)");
    BlurWideArgs a = {};
    int nsel = 0;
    for (int c = 0; c < C; ++c) {
        const double sg = sigma[c];
        if (!(sg > 0.0)) continue;  // channel not selected
        const int r = (int)(4.0 * sg + 0.5);
        MVD_REQUIRE(r <= 6, "feed_gaussian_blur_wide_f32: sigma <= 1.5 (radius int(4 sigma + 0.5) <= 6)");
        double w[13], sum = 0.0;
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
    hipLaunchKernelGGL(k_blur_axis_wide, grid, dim3(256), 0, s, x, t1, D, H, W, 0, a, 1, 0);
    int e = check_launch("feed_gaussian_blur_wide_f32");
    if (e) return e;
    hipLaunchKernelGGL(k_blur_axis_wide, grid, dim3(256), 0, s, t1, t2, D, H, W, 1, a, 0, 0);
    if ((e = check_launch("feed_gaussian_blur_wide_f32"))) return e;
    hipLaunchKernelGGL(k_blur_axis_wide, grid, dim3(256), 0, s, t2, x, D, H, W, 2, a, 0, 1);
    return check_launch("feed_gaussian_blur_wide_f32");
}

int mvd_feed_da5_apply_f32(float *x, int C, long V, int chmask, int op, const float *params, const double *stats,
                           void *stream) {
    MVD_REQUIRE(x && params, "feed_da5_apply_f32: null pointer");
    MVD_REQUIRE(C > 0 && C <= kMaxCh && chmask >= 0 && chmask < (1 << C) && V > 0,
                "feed_da5_apply_f32: bad shape (1 <= C <= 16, V > 0)");
    MVD_REQUIRE(op == kDa5Add || op == kDa5ContrastNoClip, "feed_da5_apply_f32: op is 0 (x += p) or 1 (contrast, no clip)");
    MVD_REQUIRE(op == kDa5Add || stats, "feed_da5_apply_f32: the contrast needs the channel statistics");
    ChanF p = {};
    for (int c = 0; c < C; ++c) p.v[c] = params[c];
    hipLaunchKernelGGL(k_da5_apply, dim3(stride_grid(V, 1024), C), dim3(256), 0, as_stream(stream), x, V, chmask, op, p,
                       stats);
    return check_launch("feed_da5_apply_f32");
}
}
