// Surface distances of two segmentations (medpy's __surface_distances as the reference's
// evaluation/Hausdorff.py and evaluation/metrics.py:312-382 use it): border voxels of both masks, an exact Euclidean
// distance transform to the border of one mask, gathered at the border of the other, and the fixed-order sums.
//
// The transform is three separable passes over a BOX of the volume (the bounding box of both masks: every site and
// every query lies inside it, and the distance to the nearest site does not depend on the domain it is computed in).
//   pass W: one wave per row, ballots give the nearest site left and right of every voxel;
//   pass H, pass D: one line per lane (neighbouring lanes on neighbouring W, so every access is coalesced), the lower
//           envelope of the parabolas f(j) + ((i - j) s)^2 with Meijster's integer separators; the per-line stack
//           lives in a global work buffer laid out [entry][line].
// T = int32 at unit spacing (squared voxel distances, exact), T = double with a spacing.  The separator is ESTIMATED in
// fp64 and then corrected with the same evaluated comparison that pops the stack, so a wrong estimate costs steps, not
// correctness: at unit spacing every comparison is an integer one.
#include "common.h"

namespace mvd {

constexpr int SURF_MAX_EXTENT = 1024;   // 3 * 1023^2 < 2^31, and a stack entry packs (site, start) in 2 x 16 bits
constexpr int EDT_INF_I = 0x7fffffff;   // "no site in this line so far": never squared, never added to

struct SurfBox {
    int D, H, W;      // the volume
    int lz, ly, lx;   // lower corner of the box
    int bd, bh, bw;   // its extents
};

template <typename T> __device__ __forceinline__ T edt_inf();
template <> __device__ __forceinline__ int edt_inf<int>() { return EDT_INF_I; }
template <> __device__ __forceinline__ double edt_inf<double>() { return __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ bool edt_is_inf(int v) { return v == EDT_INF_I; }
__device__ __forceinline__ bool edt_is_inf(double v) { return v == __longlong_as_double(0x7ff0000000000000LL); }

// f(j) + ((x - j) s)^2
__device__ __forceinline__ int edt_cost(int x, int j, int fj, double) { return fj + (x - j) * (x - j); }
__device__ __forceinline__ double edt_cost(int x, int j, double fj, double s) {
    const double d = (double)(x - j) * s;
    return fj + d * d;
}

// correctly rounded root of a non-negative double: one Markstein step on the library's root (a no-op where that one
// is correctly rounded already)
__device__ __forceinline__ double root_rn(double x) {
    if (!(x > 0.0) || edt_is_inf(x)) return x;
    const double r = sqrt(x);
    return fma(fma(-r, r, x), 0.5 / r, r);
}

// ------------------------------------------------------------------------------------------------------- border pass
struct LabelBitmap {
    uint32_t w[8];   // bit l: label l belongs to the set
};

template <bool I16>
__device__ __forceinline__ int surf_in_set(const void *__restrict__ v, size_t i, const uint32_t *bm) {
    const int l = I16 ? (int)reinterpret_cast<const int16_t *>(v)[i] : (int)reinterpret_cast<const uint8_t *>(v)[i];
    return (unsigned)l < 256u ? (int)((bm[l >> 5] >> (l & 31)) & 1u) : 0;
}

// 1 if voxel (z,y,x) of the mask {v in set} has a footprint neighbour that is 0 or outside the volume
template <bool I16>
__device__ __forceinline__ int surf_is_border(const void *__restrict__ v, const uint32_t *bm, int D, int H, int W, int z,
                                              int y, int x, int conn) {
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int m = (dz != 0) + (dy != 0) + (dx != 0);
                if (m == 0 || m > conn) continue;
                const int zz = z + dz, yy = y + dy, xx = x + dx;
                if ((unsigned)zz >= (unsigned)D || (unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) return 1;
                if (!surf_in_set<I16>(v, ((size_t)zz * H + yy) * W + xx, bm)) return 1;
            }
    return 0;
}

// border[v] = bit 0: v is a border voxel of mask A, bit 1: of mask B.  stats (int32[10], zeroed before the launch):
// {|A|, |B|, |border A|, |border B|, max(1024 - z), max(1024 - y), max(1024 - x), max(z + 1), max(y + 1), max(x + 1)}
// over the union of both masks -- integer atomics, one per counter and block.
template <bool A16, bool B16>
__global__ void __launch_bounds__(256) k_surf_border(const void *__restrict__ a, const void *__restrict__ b, int D, int H,
                                                     int W, LabelBitmap bmv, int conn, uint8_t *__restrict__ border,
                                                     int *__restrict__ stats) {
    __shared__ uint32_t bm[8];
    __shared__ int red[4][10];
    if (threadIdx.x < 8) bm[threadIdx.x] = bmv.w[threadIdx.x];
    __syncthreads();
    const long n = (long)D * H * W;
    int acc[10];
#pragma unroll
    for (int i = 0; i < 10; i++) acc[i] = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int ma = surf_in_set<A16>(a, (size_t)i, bm), mb = surf_in_set<B16>(b, (size_t)i, bm);
        unsigned out = 0;
        if (ma | mb) {
            const long r = i / W;
            const int x = (int)(i - r * W), z = (int)(r / H), y = (int)(r - (long)z * H);
            const int ba = ma ? surf_is_border<A16>(a, bm, D, H, W, z, y, x, conn) : 0;
            const int bb = mb ? surf_is_border<B16>(b, bm, D, H, W, z, y, x, conn) : 0;
            out = (unsigned)ba | ((unsigned)bb << 1);
            acc[0] += ma;
            acc[1] += mb;
            acc[2] += ba;
            acc[3] += bb;
            acc[4] = max(acc[4], SURF_MAX_EXTENT - z);
            acc[5] = max(acc[5], SURF_MAX_EXTENT - y);
            acc[6] = max(acc[6], SURF_MAX_EXTENT - x);
            acc[7] = max(acc[7], z + 1);
            acc[8] = max(acc[8], y + 1);
            acc[9] = max(acc[9], x + 1);
        }
        border[i] = (uint8_t)out;
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        int v = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int t = __shfl_down(v, o, 64);
            v = i < 4 ? v + t : max(v, t);
        }
        if (lane == 0) red[wid][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        const int i = threadIdx.x;
        if (i < 4) {
            const int s = red[0][i] + red[1][i] + red[2][i] + red[3][i];
            if (s) atomicAdd(stats + i, s);
        } else {
            const int s = max(max(red[0][i], red[1][i]), max(red[2][i], red[3][i]));
            if (s) atomicMax(stats + i, s);
        }
    }
}

// --------------------------------------------------------------------------------------------------------- pass W
// site: (vol[v] & bit) != 0, or == 0 when `zero_is_site`.  One wave per row of the box, four rows per block.
template <typename T>
__global__ void __launch_bounds__(256) k_edt_row(const uint8_t *__restrict__ vol, int bit, int zero_is_site, SurfBox g,
                                                 double sx, T *__restrict__ out) {
    __shared__ unsigned long long masks[4][SURF_MAX_EXTENT / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long rows = (long)g.bd * g.bh;
    const long row = (long)blockIdx.x * 4 + wid;
    const bool live = row < rows;
    const long rr = live ? row : rows - 1;
    const int z = (int)(rr / g.bh), y = (int)(rr - (long)z * g.bh);
    const uint8_t *src = vol + ((size_t)(g.lz + z) * g.H + (g.ly + y)) * g.W + g.lx;
    const int nch = (g.bw + 63) >> 6;
    for (int c = 0; c < nch; c++) {
        const int x = c * 64 + lane;
        bool site = false;
        if (x < g.bw) site = (((src[x] & bit) != 0) != (zero_is_site != 0));
        const unsigned long long m = __ballot(site);
        if (lane == 0) masks[wid][c] = m;
    }
    __syncthreads();
    if (!live) return;
    constexpr int FAR = 1 << 20;
    for (int c = 0; c < nch; c++) {
        const int x = c * 64 + lane;
        const unsigned long long m = masks[wid][c];
        int dl = FAR, dr = FAR;
        const unsigned long long ml = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        if (ml) {
            dl = lane - (63 - __clzll((long long)ml));
        } else {
            for (int cc = c - 1; cc >= 0; cc--) {
                const unsigned long long mm = masks[wid][cc];
                if (mm) {
                    dl = x - (cc * 64 + 63 - __clzll((long long)mm));
                    break;
                }
            }
        }
        const unsigned long long mr = m >> lane;
        if (mr) {
            dr = __ffsll((unsigned long long)mr) - 1;
        } else {
            for (int cc = c + 1; cc < nch; cc++) {
                const unsigned long long mm = masks[wid][cc];
                if (mm) {
                    dr = cc * 64 + (__ffsll((unsigned long long)mm) - 1) - x;
                    break;
                }
            }
        }
        const int d = min(dl, dr);
        if (x < g.bw) out[(size_t)row * g.bw + x] = d >= FAR ? edt_inf<T>() : edt_cost(d, 0, (T)0, sx);
    }
}

// ---------------------------------------------------------------------------------------------------- passes H and D
// largest x in [-1, n - 1] with cost(x, i, fi) <= cost(x, u, fu), for i < u (the difference grows with x)
template <typename T>
__device__ __forceinline__ int edt_sep(int i, T fi, int u, T fu, double s, int n) {
    const double num = ((double)fu - (double)fi) / (s * s) + (double)(u * u - i * i);
    double e = floor(num / (double)(2 * (u - i)));
    int x = e > (double)(n - 1) ? n - 1 : (e < -1.0 ? -1 : (int)e);
    while (x >= 0 && !(edt_cost(x, i, fi, s) <= edt_cost(x, u, fu, s))) x--;
    while (x < n - 1 && edt_cost(x + 1, i, fi, s) <= edt_cost(x + 1, u, fu, s)) x++;
    return x;
}

// line l: elements in[(l / inner) * outer + (l % inner) + u * stride], u < n.  stack: uint32 [n][nlines].
template <typename T>
__global__ void __launch_bounds__(256) k_edt_line(const T *__restrict__ in, T *__restrict__ out,
                                                  uint32_t *__restrict__ stack, int n, long stride, long inner, long outer,
                                                  long nlines, double s) {
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nlines) return;
    const size_t base = (size_t)(l / inner) * outer + (size_t)(l % inner);
    int q = -1, st = 0, tt = 0;
    T ft = 0;
    for (int u = 0; u < n; u++) {
        const T fu = in[base + (size_t)u * stride];
        if (edt_is_inf(fu)) continue;
        while (q >= 0 && edt_cost(tt, st, ft, s) > edt_cost(tt, u, fu, s)) {
            if (--q >= 0) {
                const uint32_t e = stack[(size_t)q * nlines + l];
                st = (int)(e & 0xffffu);
                tt = (int)(e >> 16);
                ft = in[base + (size_t)st * stride];
            }
        }
        if (q < 0) {
            q = 0;
            st = u;
            tt = 0;
            ft = fu;
            stack[l] = (uint32_t)u;
        } else {
            const int w = 1 + edt_sep<T>(st, ft, u, fu, s, n);
            if (w < n) {
                q++;
                st = u;
                tt = w;
                ft = fu;
                stack[(size_t)q * nlines + l] = (uint32_t)u | ((uint32_t)w << 16);
            }
        }
    }
    for (int u = n - 1; u >= 0; u--) {
        out[base + (size_t)u * stride] = q < 0 ? edt_inf<T>() : edt_cost(u, st, ft, s);
        if (q >= 0 && u == tt && --q >= 0) {
            const uint32_t e = stack[(size_t)q * nlines + l];
            st = (int)(e & 0xffffu);
            tt = (int)(e >> 16);
            ft = in[base + (size_t)st * stride];
        }
    }
}

// ------------------------------------------------------------------------------------------------ roots and gather
template <typename T>
__global__ void __launch_bounds__(256) k_edt_root(const T *__restrict__ sq, long n, double *__restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const T v = sq[i];
        out[i] = edt_is_inf(v) ? edt_inf<double>() : root_rn((double)v);
    }
}

// out[slot] = root of sq at the box voxels whose border byte has `bit`; slots come from an integer counter, so the
// ORDER of out is not defined (the callers sort it); a slot beyond `capacity` is counted and not written.
template <typename T>
__global__ void __launch_bounds__(256) k_surf_gather(const T *__restrict__ sq, const uint8_t *__restrict__ border, int bit,
                                                     SurfBox g, double *__restrict__ out, int capacity,
                                                     int *__restrict__ counter) {
    const long nb = (long)g.bd * g.bh * g.bw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += (long)gridDim.x * blockDim.x) {
        const long r = i / g.bw;
        const int x = (int)(i - r * g.bw), z = (int)(r / g.bh), y = (int)(r - (long)z * g.bh);
        if (border[((size_t)(g.lz + z) * g.H + (g.ly + y)) * g.W + g.lx + x] & bit) {
            const int slot = atomicAdd(counter, 1);
            const T v = sq[i];
            if (slot < capacity) out[slot] = edt_is_inf(v) ? edt_inf<double>() : root_rn((double)v);
        }
    }
}

// One block.  out = {sum s0, sum s1, s0[n0 - 1], s1[n1 - 1], all[lo], all[hi]}; the sums in a fixed order: lane t adds
// elements t, t + 1024, ... ascending, then the 1024 partials are added pairwise in a fixed tree.
__global__ void __launch_bounds__(1024) k_surf_reduce(const double *__restrict__ s0, int n0, const double *__restrict__ s1,
                                                      int n1, const double *__restrict__ all, int lo, int hi,
                                                      double *__restrict__ out) {
    __shared__ double p[2][1024];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < n0; i += 1024) a += s0[i];
    for (int i = threadIdx.x; i < n1; i += 1024) b += s1[i];
    p[0][threadIdx.x] = a;
    p[1][threadIdx.x] = b;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            p[0][threadIdx.x] += p[0][threadIdx.x + o];
            p[1][threadIdx.x] += p[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = p[0][0];
        out[1] = p[1][0];
        out[2] = s0[n0 - 1];
        out[3] = s1[n1 - 1];
        out[4] = all[lo];
        out[5] = all[hi];
    }
}

}  // namespace mvd

using namespace mvd;

static int surf_box(const char *what, SurfBox &g, int D, int H, int W, const int *box) {
    MVD_REQUIRE(D >= 1 && H >= 1 && W >= 1, "%s: empty volume", what);
    MVD_REQUIRE(D <= SURF_MAX_EXTENT && H <= SURF_MAX_EXTENT && W <= SURF_MAX_EXTENT,
                "%s: extents above %d are not built (%d x %d x %d)", what, SURF_MAX_EXTENT, D, H, W);
    MVD_REQUIRE(box, "%s: null box", what);
    const int n[3] = {D, H, W};
    for (int a = 0; a < 3; a++)
        MVD_REQUIRE(box[a] >= 0 && box[3 + a] >= 1 && box[3 + a] <= n[a] && box[a] <= n[a] - box[3 + a],
                    "%s: box [%d, %d) outside axis %d of %d", what, box[a], box[a] + box[3 + a], a, n[a]);
    g.D = D; g.H = H; g.W = W;
    g.lz = box[0]; g.ly = box[1]; g.lx = box[2];
    g.bd = box[3]; g.bh = box[4]; g.bw = box[5];
    return 0;
}

static inline unsigned surf_grid(long n) {
    long b = cdiv(n, 256);
    if (b > 8192) b = 8192;
    return (unsigned)(b < 1 ? 1 : b);
}

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

template <typename T>
static int edt_run(const uint8_t *vol, int bit, int zero_is_site, const SurfBox &g, const double *sp, void *ws,
                   hipStream_t s) {
    const size_t nb = (size_t)g.bd * g.bh * g.bw;
    T *b0 = reinterpret_cast<T *>(ws);
    T *b1 = reinterpret_cast<T *>(reinterpret_cast<char *>(ws) + align256(nb * sizeof(T)));
    uint32_t *stack = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(ws) + 2 * align256(nb * sizeof(T)));
    const long rows = (long)g.bd * g.bh;
    hipLaunchKernelGGL(k_edt_row<T>, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, vol, bit, zero_is_site, g, sp[2], b0);
    if (check_launch("edt pass W")) return 1;
    const long hw = (long)g.bh * g.bw;
    long nl = (long)g.bd * g.bw;   // pass H: line (z, x)
    hipLaunchKernelGGL(k_edt_line<T>, dim3((unsigned)cdiv(nl, 256)), dim3(256), 0, s, (const T *)b0, b1, stack, g.bh,
                       (long)g.bw, (long)g.bw, hw, nl, sp[1]);
    if (check_launch("edt pass H")) return 1;
    nl = hw;                       // pass D: line (y, x)
    hipLaunchKernelGGL(k_edt_line<T>, dim3((unsigned)cdiv(nl, 256)), dim3(256), 0, s, (const T *)b1, b0, stack, g.bd, hw,
                       hw, (long)0, nl, sp[0]);
    return check_launch("edt pass D");
}

extern "C" {

int mvd_surf_border(const void *a, int a_is_i16, const void *b, int b_is_i16, int D, int H, int W,
                    const int32_t *label_set, int nlabels, int connectivity, unsigned char *border, int32_t *stats,
                    void *stream) {
    MVD_REQUIRE(a && b && label_set && border && stats, "surf_border: null pointer");
    MVD_REQUIRE(D >= 1 && H >= 1 && W >= 1, "surf_border: empty volume");
    MVD_REQUIRE(D <= SURF_MAX_EXTENT && H <= SURF_MAX_EXTENT && W <= SURF_MAX_EXTENT,
                "surf_border: extents above %d are not built (%d x %d x %d)", SURF_MAX_EXTENT, D, H, W);
    MVD_REQUIRE(connectivity >= 1 && connectivity <= 3, "surf_border: connectivity %d not in 1..3", connectivity);
    MVD_REQUIRE(nlabels >= 1 && nlabels <= 16, "surf_border: 1..16 labels per set");
    LabelBitmap bm;
    memset(&bm, 0, sizeof(bm));
    for (int i = 0; i < nlabels; i++) {
        const int32_t l = label_set[i];
        MVD_REQUIRE(l >= 0 && l <= 255, "surf_border: label %d outside 0..255", (int)l);
        bm.w[l >> 5] |= 1u << (l & 31);
    }
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(stats, 0, 10 * sizeof(int32_t), s) != hipSuccess) {
        set_error("surf_border: memset failed");
        return 1;
    }
    const dim3 grid(surf_grid((long)D * H * W));
    if (a_is_i16 && b_is_i16)
        hipLaunchKernelGGL((k_surf_border<true, true>), grid, dim3(256), 0, s, a, b, D, H, W, bm, connectivity, border, stats);
    else if (a_is_i16)
        hipLaunchKernelGGL((k_surf_border<true, false>), grid, dim3(256), 0, s, a, b, D, H, W, bm, connectivity, border, stats);
    else if (b_is_i16)
        hipLaunchKernelGGL((k_surf_border<false, true>), grid, dim3(256), 0, s, a, b, D, H, W, bm, connectivity, border, stats);
    else
        hipLaunchKernelGGL((k_surf_border<false, false>), grid, dim3(256), 0, s, a, b, D, H, W, bm, connectivity, border, stats);
    return check_launch("surf_border");
}

size_t mvd_edt_workspace_bytes(int bd, int bh, int bw, int spaced) {
    if (bd < 1 || bh < 1 || bw < 1) return 0;
    const size_t nb = (size_t)bd * bh * bw;
    return 2 * align256(nb * (spaced ? sizeof(double) : sizeof(int32_t))) + align256(nb * sizeof(uint32_t));
}

int mvd_edt_squared(const unsigned char *vol, int bit, int zero_is_site, int D, int H, int W, const int *box,
                    const double *spacing, void *workspace, size_t workspace_bytes, void *stream) {
    MVD_REQUIRE(vol && workspace, "edt_squared: null pointer");
    MVD_REQUIRE(bit >= 1 && bit <= 255, "edt_squared: bad bit mask %d", bit);
    SurfBox g;
    if (int rc = surf_box("edt_squared", g, D, H, W, box)) return rc;
    MVD_REQUIRE(((uintptr_t)workspace & 15) == 0, "edt_squared: the workspace must be 16-byte aligned");
    MVD_REQUIRE(workspace_bytes >= mvd_edt_workspace_bytes(g.bd, g.bh, g.bw, spacing != nullptr),
                "edt_squared: workspace of %zu bytes is too small", workspace_bytes);
    hipStream_t s = as_stream(stream);
    if (spacing) {
        for (int a = 0; a < 3; a++)
            MVD_REQUIRE(spacing[a] > 0.0 && spacing[a] < 1e100, "edt_squared: spacing[%d] = %g is not positive", a, spacing[a]);
        return edt_run<double>(vol, bit, zero_is_site, g, spacing, workspace, s);
    }
    const double one[3] = {1.0, 1.0, 1.0};
    return edt_run<int>(vol, bit, zero_is_site, g, one, workspace, s);
}

int mvd_edt_root(const void *sq, int spaced, long n, double *out, void *stream) {
    MVD_REQUIRE(sq && out && n >= 1, "edt_root: null pointer or empty input");
    hipStream_t s = as_stream(stream);
    if (spaced)
        hipLaunchKernelGGL(k_edt_root<double>, dim3(surf_grid(n)), dim3(256), 0, s, (const double *)sq, n, out);
    else
        hipLaunchKernelGGL(k_edt_root<int>, dim3(surf_grid(n)), dim3(256), 0, s, (const int *)sq, n, out);
    return check_launch("edt_root");
}

int mvd_surf_gather(const void *sq, int spaced, const unsigned char *border, int bit, int D, int H, int W, const int *box,
                    double *out, int capacity, int32_t *counter, void *stream) {
    MVD_REQUIRE(sq && border && out && counter, "surf_gather: null pointer");
    MVD_REQUIRE(bit >= 1 && bit <= 255 && capacity >= 1, "surf_gather: bad bit mask or capacity");
    SurfBox g;
    if (int rc = surf_box("surf_gather", g, D, H, W, box)) return rc;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(counter, 0, sizeof(int32_t), s) != hipSuccess) {
        set_error("surf_gather: memset failed");
        return 1;
    }
    const dim3 grid(surf_grid((long)g.bd * g.bh * g.bw));
    if (spaced)
        hipLaunchKernelGGL(k_surf_gather<double>, grid, dim3(256), 0, s, (const double *)sq, border, bit, g, out, capacity,
                           counter);
    else
        hipLaunchKernelGGL(k_surf_gather<int>, grid, dim3(256), 0, s, (const int *)sq, border, bit, g, out, capacity, counter);
    return check_launch("surf_gather");
}

int mvd_surf_reduce(const double *s0, int n0, const double *s1, int n1, const double *all, int lo, int hi, double *out,
                    void *stream) {
    MVD_REQUIRE(s0 && s1 && all && out, "surf_reduce: null pointer");
    MVD_REQUIRE(n0 >= 1 && n1 >= 1, "surf_reduce: empty surface");
    MVD_REQUIRE(lo >= 0 && hi >= lo && (long)hi < (long)n0 + n1, "surf_reduce: order statistics [%d, %d] outside %ld values",
                lo, hi, (long)n0 + n1);
    hipLaunchKernelGGL(k_surf_reduce, dim3(1), dim3(1024), 0, as_stream(stream), s0, n0, s1, n1, all, lo, hi, out);
    return check_launch("surf_reduce");
}
}
