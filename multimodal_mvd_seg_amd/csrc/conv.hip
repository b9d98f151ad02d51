// Conv3d / ConvTranspose3d entry points: geometry set-up, engine dispatch (MFMA implicit GEMM when the shape allows,
// scalar gather kernels otherwise) and the scalar engines themselves.
#include "common.h"
#include "conv_geom.h"

namespace mvd {

static int g_engine_mode = 0;  // 0 auto, 1 scalar only
// Winograd F(2,3) engine switches (debug): MVD_WINO=0 disables it, MVD_WINO_MIN overrides the minimum number of
// 128-voxel x 32-channel work items below which the direct engines (which can split the reduction) are used
#define g_wino_off (wino_mode() == 0)
// MVD_TRANSP=0: transposed convs through the gathered-tap engines (debug / A-B)
static const int g_transp_off = getenv("MVD_TRANSP") ? (atoi(getenv("MVD_TRANSP")) == 0) : 0;
static long g_wino_min_items = getenv("MVD_WINO_MIN") ? atol(getenv("MVD_WINO_MIN")) : 256;
// the F(2x2x2,3x3x3) engine (MVD_WINO3=0: off) takes a Winograd layer when it has at least this many 4x8x8-voxel x
// 32-channel work items PER SAMPLE (one workgroup per CU).  Per sample, so that the engine of a layer does not depend on
// the batch size: a data-parallel step (one sample per rank) then runs the engines of the single-process step.
// Measured it beats k_fwd_wino2 on every stride-1 layer of the flagship down to 16^3 x 256 channels = 128 items per
// sample
static const long kWino3MinItemsDefault = 128;
static long g_wino3_min_items = getenv("MVD_WINO3_MIN") ? atol(getenv("MVD_WINO3_MIN")) : kWino3MinItemsDefault;
// the F(2x2,3x3) engine of the 9-tap 1x3x3 layers (conv_wino2p.hip) takes a layer with at least this many work items (4 planes
// x 4 x 8 outputs x 32 channels, over all N * D planes: its tile spans samples when D = 1); MVD_WINO2P_MIN overrides
static const long kWino2pMinItemsDefault = 256;
static long g_wino2p_min_items = getenv("MVD_WINO2P_MIN") ? atol(getenv("MVD_WINO2P_MIN")) : kWino2pMinItemsDefault;

// ----------------------------------------------------------------------------------------- fp32 Winograd engine route
// One forward-type pass as the engine predicates see it: output grid, the parts of its reduce and of its produce channels
// (forward: C1, C2 -> K; input gradient: K -> C1, C2), kernel size and stride of the conv
struct ConvPass {
    int N, D, H, W, R1, R2, P1, P2;
    const int *ks, *st;
};
static ConvPass fwd_pass(int N, int D, int H, int W, int C1, int C2, int K, const int ks[3], const int st[3]) {
    return {N, D, H, W, C1, C2, K, 0, ks, st};
}
static ConvPass dgrad_pass(int N, int D, int H, int W, int C1, int C2, int K, const int ks[3], const int st[3]) {
    return {N, D, H, W, K, 0, C1, C2, ks, st};
}
// what the three engines share: engines on, a kd x 3 x 3 stride-1 conv, every channel part a multiple of 32
static bool wino_pass_ok(const ConvPass &p, int kd) {
    if (g_engine_mode != 0 || g_wino_off || !p.ks || !p.st) return false;
    if (p.ks[0] != kd || p.ks[1] != 3 || p.ks[2] != 3 || p.st[0] != 1 || p.st[1] != 1 || p.st[2] != 1) return false;
    if (p.N <= 0 || p.D <= 0 || p.H <= 0 || p.W <= 0 || p.R1 <= 0 || p.R2 < 0 || p.P1 <= 0 || p.P2 < 0) return false;
    return !(p.R1 % 32 || p.R2 % 32 || p.P1 % 32 || p.P2 % 32);
}
// "would engine E take this pass?" -- asked by the mvd_conv_*_applicable queries, by mvd_conv3d_route and by run_fwd, each
// with the engine's work-item count next to it
static long wino2_items(int N, int D, int H, int W, int K) { return (long)N * ((D + 3) / 4) * ((H + 3) / 4) * ((W + 7) / 8) * (K / 32); }
static bool wino2_takes(const ConvPass &p) {
    return wino_pass_ok(p, 3) && wino2_items(p.N, p.D, p.H, p.W, p.P1 + p.P2) >= g_wino_min_items;
}
static long wino3_items(int D, int H, int W, int K) { return (long)((D + 3) / 4) * ((H + 7) / 8) * ((W + 7) / 8) * (K / 32); }
static bool wino3_takes(const ConvPass &p) {  // a refinement of F(2x2,3x3): that engine's minimum holds too
    return wino3_enabled() && wino2_takes(p) && wino3_items(p.D, p.H, p.W, p.P1 + p.P2) >= g_wino3_min_items;
}
static bool wino2p_takes(const ConvPass &p) {
    if (!wino_pass_ok(p, 1)) return false;
    const int cmax = p.R1 + p.R2 > p.P1 + p.P2 ? p.R1 + p.R2 : p.P1 + p.P2;
    if ((long)p.H * p.W * cmax * 4 >= (1L << 31) || (long)p.N * p.D > (1L << 30)) return false;
    return wino2p_items(p.N, p.D, p.H, p.W, p.P1 + p.P2) >= g_wino2p_min_items;
}
static bool engine_takes(int kind, const ConvPass &p) {
    return kind == MVD_CONV_WINO3 ? wino3_takes(p) : kind == MVD_CONV_WINO2 ? wino2_takes(p) : kind == MVD_CONV_WINO2P && wino2p_takes(p);
}
// the preferred engine of a pass: the 3-D engine over F(2x2,3x3), the in-plane engine for 1x3x3, direct otherwise
static int route_of(const ConvPass &p) {
    return wino3_takes(p) ? MVD_CONV_WINO3 : wino2_takes(p) ? MVD_CONV_WINO2 : wino2p_takes(p) ? MVD_CONV_WINO2P : MVD_CONV_DIRECT;
}
// a Winograd-domain weight table and the engine it belongs to (u == nullptr: none), with the conv's kernel size and stride
struct WinoTable {
    const float *u;
    int kind;
    const int *ks, *st;
};

// =============================================================================================== scalar forward-type
// one thread per (n, o, k); k fastest so weight reads and output writes are coalesced and A is a wave broadcast
__global__ void k_fwd_scalar(FwdGeom g, const float *__restrict__ a1, const float *__restrict__ a2,
                             const float *__restrict__ w, const float *__restrict__ bias, float *__restrict__ y1,
                             float *__restrict__ y2) {
    const int K = g.K1 + g.K2, C = g.C1 + g.C2;
    const int CK = wl_ck(C);
    const long total = (long)g.N * g.Do * g.Ho * g.Wo * K;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        int k = (int)(idx % K);
        long r = idx / K;
        int ow = (int)(r % g.Wo);
        r /= g.Wo;
        int oh = (int)(r % g.Ho);
        r /= g.Ho;
        int od = (int)(r % g.Do);
        int n = (int)(r / g.Do);
        float acc = bias ? bias[k] : 0.f;
        for (int t = 0; t < g.ntaps; t++) {
            int id = od * g.sa[0] + g.off[t][0], ih = oh * g.sa[1] + g.off[t][1], iw = ow * g.sa[2] + g.off[t][2];
            if (id < 0 || id >= g.Di || ih < 0 || ih >= g.Hi || iw < 0 || iw >= g.Wi) continue;
            size_t vox = (((size_t)n * g.Di + id) * g.Hi + ih) * g.Wi + iw;
            const int tw = g.wt[t];
            const float *p1 = a1 + vox * g.C1;
            for (int c = 0; c < g.C1; c++) acc += p1[c] * w[widx(CK, g.T, C, K, tw, c, k)];
            if (g.C2) {
                const float *p2 = a2 + vox * g.C2;
                for (int c = 0; c < g.C2; c++) acc += p2[c] * w[widx(CK, g.T, C, K, tw, g.C1 + c, k)];
            }
        }
        size_t ov = (((size_t)n * g.Dy + (od * g.so[0] + g.oo[0])) * g.Hy + (oh * g.so[1] + g.oo[1])) * g.Wy +
                    (ow * g.so[2] + g.oo[2]);
        if (k < g.K1)
            y1[ov * g.K1 + k] = acc;
        else
            y2[ov * g.K2 + (k - g.K1)] = acc;
    }
}

int fwd_scalar(const FwdGeom &g, const float *a1, const float *a2, const float *w, const float *bias, float *y1,
               float *y2, hipStream_t s) {
    long total = (long)g.N * g.Do * g.Ho * g.Wo * (g.K1 + g.K2);
    if (total <= 0) return 0;
    long blocks = cdiv(total, 256);
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_fwd_scalar, dim3(blocks), dim3(256), 0, s, g, a1, a2, w, bias, y1, y2);
    return check_launch("conv fwd (scalar)");
}

// =============================================================================================== scalar wgrad-type
// grid (ceil(ntaps*C*K/256), nsplit): each thread owns one (t,c,k) and a slice of the voxels; fp64 partials,
// fixed-order second stage.
__global__ void k_wgrad_scalar(WgradGeom g, const float *__restrict__ a1, const float *__restrict__ a2,
                               const float *__restrict__ b, double *__restrict__ partial, long chunk) {
    const int C = g.C1 + g.C2, K = g.K;
    const long per = (long)g.ntaps * C * K;
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= per) return;
    const int k = (int)(j % K);
    const int c = (int)((j / K) % C);
    const int t = (int)(j / ((long)K * C));
    const long total = (long)g.N * g.Do * g.Ho * g.Wo;
    const long v0 = (long)blockIdx.y * chunk;
    long v1 = v0 + chunk;
    if (v1 > total) v1 = total;
    double acc = 0.0;
    for (long v = v0; v < v1; v++) {
        long r = v;
        int ow = (int)(r % g.Wo);
        r /= g.Wo;
        int oh = (int)(r % g.Ho);
        r /= g.Ho;
        int od = (int)(r % g.Do);
        int n = (int)(r / g.Do);
        int id = od * g.sa[0] + g.off[t][0], ih = oh * g.sa[1] + g.off[t][1], iw = ow * g.sa[2] + g.off[t][2];
        if (id < 0 || id >= g.Di || ih < 0 || ih >= g.Hi || iw < 0 || iw >= g.Wi) continue;
        int bd = od * g.sb[0] + g.ob[t][0], bh = oh * g.sb[1] + g.ob[t][1], bw = ow * g.sb[2] + g.ob[t][2];
        if (bd < 0 || bd >= g.Db || bh < 0 || bh >= g.Hb || bw < 0 || bw >= g.Wb) continue;
        size_t va = (((size_t)n * g.Di + id) * g.Hi + ih) * g.Wi + iw;
        size_t vb = (((size_t)n * g.Db + bd) * g.Hb + bh) * g.Wb + bw;
        float av = c < g.C1 ? a1[va * g.C1 + c] : a2[va * g.C2 + (c - g.C1)];
        acc += (double)(av * b[vb * K + k]);
    }
    partial[(size_t)blockIdx.y * per + j] = acc;
}

// dw[torch layout] = sum_split partial[split][t][c][k]
__global__ void k_wgrad_reduce_d(WgradGeom g, const double *__restrict__ partial, float *__restrict__ dw, int nsplit) {
    const int C = g.C1 + g.C2, K = g.K;
    const long per = (long)g.ntaps * C * K;
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= per) return;
    double s = 0;
    for (int b = 0; b < nsplit; b++) s += partial[(size_t)b * per + j];
    const int k = (int)(j % K);
    const int c = (int)((j / K) % C);
    const int t = g.wt[(int)(j / ((long)K * C))];
    size_t o = g.transposed_out ? ((size_t)c * K + k) * g.T + t : ((size_t)k * C + c) * g.T + t;
    dw[o] = (float)s;
}

int wgrad_scalar_split(const WgradGeom &g, long *chunk) {
    long total = (long)g.N * g.Do * g.Ho * g.Wo;
    long per = (long)g.ntaps * (g.C1 + g.C2) * g.K;
    long nsplit = cdiv(total, 512);
    long cap = (64L << 20) / (per * 8);  // keep the partial buffer <= 64 MiB
    if (cap < 1) cap = 1;
    if (nsplit > cap) nsplit = cap;
    if (nsplit > 256) nsplit = 256;
    if (nsplit < 1) nsplit = 1;
    *chunk = cdiv(total, nsplit);
    return (int)cdiv(total, *chunk);
}

size_t wgrad_scalar_ws(const WgradGeom &g) {
    long chunk;
    int ns = wgrad_scalar_split(g, &chunk);
    return (size_t)ns * g.ntaps * (g.C1 + g.C2) * g.K * sizeof(double) + 256;
}

int wgrad_scalar(const WgradPlan &p, const WgradGeom &g, const float *a1, const float *a2, const float *b, float *dw, void *ws,
                 hipStream_t s) {
    const long chunk = p.chunk;
    const int ns = p.nsplit;
    MVD_REQUIRE(p.ws_bytes >= p.needed_ws, "conv wgrad (scalar): workspace too small");
    long per = (long)g.ntaps * (g.C1 + g.C2) * g.K;
    double *partial = reinterpret_cast<double *>(ws);
    g_wgrad_last_kernel = WG_SCALAR;
    hipLaunchKernelGGL(k_wgrad_scalar, dim3(cdiv(per, 256), ns), dim3(256), 0, s, g, a1, a2, b, partial, chunk);
    if (check_launch("conv wgrad (scalar)")) return 1;
    hipLaunchKernelGGL(k_wgrad_reduce_d, dim3(cdiv(per, 256)), dim3(256), 0, s, g, partial, dw, ns);
    return check_launch("conv wgrad reduce");
}

// =============================================================================================== bias gradient
// dbias[k] = sum over rows of dy[rows][K]
__global__ void k_colsum(const float *__restrict__ x, double *__restrict__ partial, long rows, int K, long chunk) {
    __shared__ double sm[256];
    const int t = threadIdx.x;
    const long r0 = (long)blockIdx.x * chunk;
    long r1 = r0 + chunk;
    if (r1 > rows) r1 = rows;
    if (K <= 256) {
        const int R = 256 / K;  // rows in flight; lanes walk a row contiguously
        const int k = t % K, r = t / K;
        double acc = 0;
        if (r < R)
            for (long i = r0 + r; i < r1; i += R) acc += (double)x[(size_t)i * K + k];
        sm[t] = (r < R) ? acc : 0.0;
        __syncthreads();
        if (t < K) {
            double s = 0;
            for (int rr = 0; rr < R; rr++) s += sm[rr * K + t];
            partial[(size_t)blockIdx.x * K + t] = s;
        }
    } else {
        for (int kk = t; kk < K; kk += 256) {
            double acc = 0;
            for (long i = r0; i < r1; i++) acc += (double)x[(size_t)i * K + kk];
            partial[(size_t)blockIdx.x * K + kk] = acc;
        }
    }
}

// K % 4 == 0, K <= 1024: float4 loads, several rows in flight per thread (HBM-bound streaming pass)
template <bool BF>
__global__ void k_colsum4(const float *__restrict__ x, double *__restrict__ partial, long rows, int K, long chunk) {
    extern __shared__ double sm4[];  // [R][K]
    const int t = threadIdx.x;
    const int KG = K / 4;
    const int R = blockDim.x / KG;
    const int g = t % KG, r = t / KG;
    const long r0 = (long)blockIdx.x * chunk;
    long r1 = r0 + chunk;
    if (r1 > rows) r1 = rows;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    if (r < R) {
        auto ld = [&](long row) -> float4 {
            if (BF) {
                const uint2 q = *reinterpret_cast<const uint2 *>(reinterpret_cast<const unsigned short *>(x) + (size_t)row * K + g * 4);
                return make_float4(__uint_as_float(q.x << 16), __uint_as_float(q.x & 0xffff0000u), __uint_as_float(q.y << 16),
                                   __uint_as_float(q.y & 0xffff0000u));
            }
            return *reinterpret_cast<const float4 *>(x + (size_t)row * K + g * 4);
        };
        long i = r0 + r;
        for (; i + 3L * R < r1; i += 4L * R) {
            float4 q0 = ld(i);
            float4 q1 = ld(i + R);
            float4 q2 = ld(i + 2L * R);
            float4 q3 = ld(i + 3L * R);
            a0 += (double)((q0.x + q1.x) + (q2.x + q3.x));
            a1 += (double)((q0.y + q1.y) + (q2.y + q3.y));
            a2 += (double)((q0.z + q1.z) + (q2.z + q3.z));
            a3 += (double)((q0.w + q1.w) + (q2.w + q3.w));
        }
        for (; i < r1; i += R) {
            float4 q = ld(i);
            a0 += (double)q.x; a1 += (double)q.y; a2 += (double)q.z; a3 += (double)q.w;
        }
        double *o = sm4 + (size_t)r * K + g * 4;
        o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3;
    }
    __syncthreads();
    for (int k = t; k < K; k += blockDim.x) {
        double s = 0;
        for (int rr = 0; rr < R; rr++) s += sm4[(size_t)rr * K + k];
        partial[(size_t)blockIdx.x * K + k] = s;
    }
}

static int colsum_blocks(long rows, long *chunk) {
    long nb = rows / 256;
    if (nb < 1) nb = 1;
    if (nb > 2048) nb = 2048;
    *chunk = cdiv(rows, nb);
    return (int)cdiv(rows, *chunk);
}
static size_t colsum_ws(long rows, int K) {
    long chunk;
    return (size_t)colsum_blocks(rows, &chunk) * K * sizeof(double) + 256;
}
static int colsum(const float *x, float *out, long rows, int K, void *ws, hipStream_t s, bool bf = false) {
    long chunk;
    int nb = colsum_blocks(rows, &chunk);
    double *partial = reinterpret_cast<double *>(ws);
    if (K % 4 == 0 && K <= 1024 && (((uintptr_t)x) & 15) == 0) {
        const int KG = K / 4;
        const int R = 256 / KG > 0 ? 256 / KG : 1;
        const int threads = (R * KG + 63) / 64 * 64;
        if (bf)
            hipLaunchKernelGGL(k_colsum4<true>, dim3(nb), dim3(threads), (size_t)R * K * sizeof(double), s, x, partial, rows,
                               K, chunk);
        else
            hipLaunchKernelGGL(k_colsum4<false>, dim3(nb), dim3(threads), (size_t)R * K * sizeof(double), s, x, partial, rows,
                               K, chunk);
    } else if (bf) {
        set_error("bias grad (bf16): K %% 4 != 0 is not supported");
        return 2;
    } else {
        hipLaunchKernelGGL(k_colsum, dim3(nb), dim3(256), 0, s, x, partial, rows, K, chunk);
    }
    if (check_launch("bias grad")) return 1;
    return reduce_partials(partial, out, nb, K, s);
}

// =============================================================================================== engine dispatch
// (the geometry builders are in conv_geom.h)
static int check_ks(const int ks[3], const int st[3], const char *who) {
    for (int a = 0; a < 3; a++) {
        if (!(ks[a] == 1 || ks[a] == 3)) {
            set_error("%s: kernel size must be 1 or 3 per axis (got %d)", who, ks[a]);
            return 1;
        }
        if (!(st[a] == 1 || st[a] == 2)) {
            set_error("%s: stride must be 1 or 2 per axis (got %d)", who, st[a]);
            return 1;
        }
    }
    return 0;
}
// the shape queries: 0 / "no" for arguments the entry points would refuse
static bool conv_args_ok(int N, int D, int H, int W, int C1, int C2, int K, const int ks[3], const int st[3], const char *who) {
    return N > 0 && D > 0 && H > 0 && W > 0 && C1 > 0 && C2 >= 0 && K > 0 && ks && st && !check_ks(ks, st, who);
}

// tab (optional): a Winograd table of this pass (uf of the forward, ub of the input gradient).  Its engine runs if and only
// if that engine's predicate holds for the pass; the direct engines run otherwise, and when the engine itself refuses (-1)
static int run_fwd(const FwdGeom &g, const float *a1, const float *a2, const float *w, const float *bias, float *y1,
                   float *y2, void *ws, size_t ws_bytes, hipStream_t s, const WinoTable *tab = nullptr, float *stats = nullptr,
                   int *stats_done = nullptr, long direct_tiles = 0) {
    if (stats_done) *stats_done = 0;
    if (direct_tiles > 0) {  // statistics from the direct engine's epilogue ([N][direct_tiles][K][2], fwd_mfma)
        if (g_engine_mode == 0) {
            int r = fwd_mfma(g, a1, a2, w, bias, y1, y2, ws, ws_bytes, s, stats, direct_tiles, stats_done);
            if (r >= 0) return r;
            if (stats_done) *stats_done = 0;
        }
        return fwd_scalar(g, a1, a2, w, bias, y1, y2, s);
    }
    if (tab && tab->u && engine_takes(tab->kind, ConvPass{g.N, g.Do, g.Ho, g.Wo, g.C1, g.C2, g.K1, g.K2, tab->ks, tab->st})) {
        int r = tab->kind == MVD_CONV_WINO3   ? fwd_wino3(g, a1, a2, tab->u, bias, y1, y2, s, stats, stats_done)
                : tab->kind == MVD_CONV_WINO2 ? fwd_wino(g, a1, a2, tab->u, bias, y1, y2, s, stats, stats_done)
                                              : fwd_wino2p(g, a1, a2, tab->u, bias, y1, y2, s);
        if (r >= 0) return r;
        if (stats_done) *stats_done = 0;
    }
    if (g_engine_mode == 0) {
        int r = fwd_mfma(g, a1, a2, w, bias, y1, y2, ws, ws_bytes, s);
        if (r >= 0) return r;
    }
    return fwd_scalar(g, a1, a2, w, bias, y1, y2, s);
}

int conv_engine_mode() { return g_engine_mode; }

// the MFMA kernels read 16 bytes at a time: other pointers take the scalar kernel (fp32) or are refused (bf16)
static bool wgrad_aligned(const void *a1, const void *a2, const void *b) {
    return (((uintptr_t)a1 | (uintptr_t)a2 | (uintptr_t)b) & 15) == 0;
}

static int run_wgrad(const WgradGeom &g, const float *a1, const float *a2, const float *b, float *dw, void *ws,
                     size_t ws_bytes, hipStream_t s, float *dbias = nullptr, int *dbias_done = nullptr) {
    if (dbias_done) *dbias_done = 0;
    WgradPlan p;
    int r = wgrad_plan(g, false, ws_bytes, dbias && dbias_done, false, &p);
    if (r) return r;
    if (p.kernel != WG_SCALAR && !wgrad_aligned(a1, a2, b)) wgrad_plan_scalar(g, ws_bytes, dbias && dbias_done, &p);
    return wgrad_launch(p, g, a1, a2, b, dw, ws, s, dbias, dbias_done);
}

static int run_fwd16(const FwdGeom &g, const uint16_t *a1, const uint16_t *a2, const uint16_t *w, const float *bias,
                     uint16_t *y1, uint16_t *y2, void *ws, size_t ws_bytes, hipStream_t s, const Fwd16Fuse *fuse = nullptr) {
    int r = fwd_bf16(g, a1, a2, w, bias, y1, y2, ws, ws_bytes, s, fuse);
    if (r < 0 && fuse && fuse->in_scale) {
        set_error("bf16 conv engine: the fused InstanceNorm input prologue needs the z-marching kernel (3x3x3 stride 1, 32 -> 32 "
                  "channels, >= 4 tiles per CU); C=%d+%d K=%d+%d", g.C1, g.C2, g.K1, g.K2);
        return 3;
    }
    if (r < 0) {
        set_error("bf16 conv engine: unsupported shape (needs C %% 32 == 0 and K %% 32 == 0; C=%d+%d K=%d+%d)", g.C1, g.C2,
                  g.K1, g.K2);
        return 3;
    }
    return r;
}

static int run_wgrad16(const WgradGeom &g, const uint16_t *a1, const uint16_t *a2, const uint16_t *b, float *dw, void *ws,
                       size_t ws_bytes, hipStream_t s, float *dbias = nullptr, int *dbias_done = nullptr) {
    if (dbias_done) *dbias_done = 0;
    WgradPlan p;
    int r = wgrad_plan(g, true, ws_bytes, dbias && dbias_done, false, &p);
    if (r == 3 || (r == 0 && !wgrad_aligned(a1, a2, b))) {
        set_error("bf16 wgrad: unsupported shape (needs C %% 32 == 0 and K %% 32 == 0; C=%d+%d K=%d)", g.C1, g.C2, g.K);
        return 3;
    }
    if (r) return r;
    return wgrad_launch(p, g, reinterpret_cast<const float *>(a1), reinterpret_cast<const float *>(a2),
                        reinterpret_cast<const float *>(b), dw, ws, s, dbias, dbias_done);
}

static size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

}  // namespace mvd

using namespace mvd;

extern "C" {

int mvd_set_conv_engine(int mode) {
    g_engine_mode = mode ? 1 : 0;
    return 0;
}

int mvd_set_wino_min_items(long n) {
    g_wino_min_items = n < 0 ? 256 : n;
    return 0;
}

size_t mvd_conv_fwd_workspace_bytes(int N, long out_voxels, int K) { return fwd_mfma_ws(N, out_voxels, K); }

/* The general fp32 forward.  table / table_kind: a Winograd table of the weight and the engine it is for (MVD_CONV_*;
 * NULL: none).  stats == NULL: no statistics epilogue; stats_tiles == 0: that of the Winograd engines (the 4x4x8-tile layout
 * of mvd_conv_stats_tiles); stats_tiles > 0: that of the direct engines (mvd_conv3d_fwd_stats_tiles; the table is not used) */
int mvd_conv3d_fwd_routed(const float *x1, int C1, const float *x2, int C2, const float *wf, const float *table, int table_kind,
                          const float *bias, float *y, float *stats, long stats_tiles, int *stats_done, int N, int D, int H,
                          int W, int K, const int ksize[3], const int stride[3], void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(x1 && wf && y && C1 > 0 && C2 >= 0 && (C2 == 0 || x2), "conv3d_fwd: null pointer / bad channels");
    MVD_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && K > 0, "conv3d_fwd: bad shape");
    if (check_ks(ksize, stride, "conv3d_fwd")) return 2;
    MVD_REQUIRE(table_kind >= MVD_CONV_DIRECT && table_kind <= MVD_CONV_WINO2P, "conv3d_fwd: unknown table kind");
    MVD_REQUIRE(!(table && table_kind == MVD_CONV_WINO2P) || (ksize[0] == 1 && ksize[1] == 3 && ksize[2] == 3),
                "conv3d_fwd: the in-plane table is that of a 1x3x3 kernel");
    MVD_REQUIRE(!stats || stats_done, "conv3d_fwd: stats_done is required with stats");
    MVD_REQUIRE(stats_tiles == 0 || (stats && stats_tiles > 0), "conv3d_fwd: stats_tiles > 0 comes with stats and stats_done");
    FwdGeom g;
    conv_fwd_geom(g, N, D, H, W, C1, C2, K, ksize, stride);
    const WinoTable tab = {table, table_kind, ksize, stride};
    return run_fwd(g, x1, x2, wf, bias, y, nullptr, ws, ws_bytes, as_stream(stream), &tab, stats, stats_done, stats_tiles);
}

int mvd_conv3d_fwd(const float *x1, int C1, const float *x2, int C2, const float *wf, const float *bias, float *y, int N,
                   int D, int H, int W, int K, const int ksize[3], const int stride[3], void *ws, size_t ws_bytes,
                   void *stream) {
    return mvd_conv3d_fwd_routed(x1, C1, x2, C2, wf, nullptr, MVD_CONV_DIRECT, bias, y, nullptr, 0, nullptr, N, D, H, W, K, ksize,
                                 stride, ws, ws_bytes, stream);
}

int mvd_conv3d_fwd_wino(const float *x1, int C1, const float *x2, int C2, const float *wf, const float *uf,
                        const float *bias, float *y, int N, int D, int H, int W, int K, const int ksize[3],
                        const int stride[3], void *ws, size_t ws_bytes, void *stream) {
    return mvd_conv3d_fwd_routed(x1, C1, x2, C2, wf, uf, uf ? MVD_CONV_WINO2 : MVD_CONV_DIRECT, bias, y, nullptr, 0, nullptr, N, D, H,
                                 W, K, ksize, stride, ws, ws_bytes, stream);
}

/* forward (1) | input gradient (2) bits: the engine would take that pass with its table (the caller can skip packing the
 * table otherwise) */
static int pass_bits(bool (*takes)(const ConvPass &), int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3],
                     const int stride[3]) {
    return (takes(fwd_pass(N, D, H, W, C1, C2, K, ksize, stride)) ? 1 : 0) |
           (takes(dgrad_pass(N, D, H, W, C1, C2, K, ksize, stride)) ? 2 : 0);
}
int mvd_conv_wino_applicable(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3], const int stride[3]) {
    return pass_bits(wino2_takes, N, D, H, W, C1, C2, K, ksize, stride);
}
int mvd_conv_wino3_applicable(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3], const int stride[3]) {
    return pass_bits(wino3_takes, N, D, H, W, C1, C2, K, ksize, stride);
}
int mvd_conv_wino2p_applicable(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3], const int stride[3]) {
    return pass_bits(wino2p_takes, N, D, H, W, C1, C2, K, ksize, stride);
}
/* the preferred engine (MVD_CONV_*) of the forward in bits 0-3 and of the input gradient in bits 4-7 */
int mvd_conv3d_route(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3], const int stride[3]) {
    return route_of(fwd_pass(N, D, H, W, C1, C2, K, ksize, stride)) | (route_of(dgrad_pass(N, D, H, W, C1, C2, K, ksize, stride)) << 4);
}

size_t mvd_wino_weight_elems(int C, int K) { return wino_weight_elems(C, K); }
int mvd_wino_mode(void) { return wino_mode(); }

/* InstanceNorm statistics epilogue: tiles per sample of the partial-statistics buffer [N][tiles][K][2] floats */
size_t mvd_conv_stats_tiles(int D, int H, int W) { return (size_t)((D + 3) / 4) * ((H + 3) / 4) * ((W + 7) / 8); }

/* The direct fp32 engines' statistics epilogue (the narrow-input / chunked kernel and the stride-2 kernel): tiles per sample
 * of the kernel that would run for this conv, 0 when it has none (Winograd layers take theirs with stats_tiles = 0) */
long mvd_conv3d_fwd_stats_tiles(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3], const int stride[3]) {
    if (g_engine_mode != 0 || !conv_args_ok(N, D, H, W, C1, C2, K, ksize, stride, "conv3d_fwd_stats_tiles")) return 0;
    FwdGeom g;
    conv_fwd_geom(g, N, D, H, W, C1, C2, K, ksize, stride);
    long tiles = 0;
    // (alignment of the tensors is checked at the call; the pointers here only have to be non-null and aligned)
    const float *al = reinterpret_cast<const float *>(uintptr_t(64));
    if (fwd_mfma(g, al, C2 ? al : nullptr, al, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, &tiles) != 0)
        return 0;
    return tiles;
}

int mvd_pack_weight_wino(const float *w, float *uf, float *ub, int K, int C, void *stream) {
    MVD_REQUIRE(w && (uf || ub) && K > 0 && C > 0, "pack_weight_wino: bad arguments");
    MVD_REQUIRE(K % 32 == 0 && C % 32 == 0, "pack_weight_wino: needs C %% 32 == 0 and K %% 32 == 0");
    return pack_weight_wino(w, uf, ub, K, C, as_stream(stream));
}

// ------------------------------------------------------------------------------------- F(2x2x2,3x3x3) engine (3-D)
int mvd_set_wino3_min_items(long n) {
    g_wino3_min_items = n < 0 ? kWino3MinItemsDefault : n;
    return 0;
}

size_t mvd_wino3_weight_elems(int C, int K) { return (size_t)64 * C * K; }

int mvd_pack_weight_wino3(const float *w, float *uf, float *ub, int K, int C, void *stream) {
    MVD_REQUIRE(w && (uf || ub) && K > 0 && C > 0, "pack_weight_wino3: bad arguments");
    MVD_REQUIRE(K % 32 == 0 && C % 32 == 0, "pack_weight_wino3: needs C %% 32 == 0 and K %% 32 == 0");
    return pack_weight_wino3(w, uf, ub, K, C, as_stream(stream));
}

int mvd_pack_weights_batch3(int n, const float *const *w, float *const *wf, float *const *wb, float *const *uf,
                            float *const *ub, float *const *vf, float *const *vb, const int *K, const int *C,
                            const int *T, const int *transposed, void *stream) {
    MVD_REQUIRE(n > 0 && w && wf && wb && uf && ub && vf && vb && K && C && T && transposed,
                "pack_weights_batch3: null table");
    for (int q = 0; q < n; q++) {
        MVD_REQUIRE(w[q] && (wf[q] || wb[q] || uf[q] || ub[q] || vf[q] || vb[q]),
                    "pack_weights_batch3: job without source or destination");
        MVD_REQUIRE(K[q] > 0 && C[q] > 0 && T[q] > 0 && T[q] <= MVD_MAX_TAPS, "pack_weights_batch3: bad K / C / T");
        if (uf[q] || ub[q]) MVD_REQUIRE(wino_mode() == 2, "pack_weights_batch3: Winograd tables need MVD_WINO=2");
        // T = 9: uf / ub are the F(2x2,3x3) tables of a 1x3x3 layer (mvd_pack_weight_wino2p); the caller passes them for
        // that kernel shape only
        if (uf[q] || ub[q] || vf[q] || vb[q])
            MVD_REQUIRE((T[q] == 27 || (T[q] == 9 && !vf[q] && !vb[q])) && !transposed[q] && K[q] % 32 == 0 && C[q] % 32 == 0,
                        "pack_weights_batch3: Winograd tables need a 3x3x3 (or, uf / ub, 1x3x3) conv with C %% 32 == 0 and K %% 32 == 0");
    }
    return pack_weights_batch(n, w, wf, wb, uf, ub, K, C, T, transposed, as_stream(stream), vf, vb);
}

// ------------------------------------------------------------------------------------- F(2x2,3x3) engine of 1x3x3 layers
int mvd_set_wino2p_min_items(long n) {
    g_wino2p_min_items = n < 0 ? kWino2pMinItemsDefault : n;
    return 0;
}

size_t mvd_wino2p_weight_elems(int C, int K) { return (size_t)16 * C * K; }

int mvd_pack_weight_wino2p(const float *w, float *uf, float *ub, int K, int C, void *stream) {
    MVD_REQUIRE(w && (uf || ub) && K > 0 && C > 0, "pack_weight_wino2p: bad arguments");
    MVD_REQUIRE(K % 32 == 0 && C % 32 == 0, "pack_weight_wino2p: needs C %% 32 == 0 and K %% 32 == 0");
    return pack_weight_wino2p(w, uf, ub, K, C, as_stream(stream));
}

// ------------------------------------------------------------------------------------------------ input gradient
static bool k3s2(const int ks[3], const int st[3]) {
    return ks[0] == 3 && ks[1] == 3 && ks[2] == 3 && st[0] == 2 && st[1] == 2 && st[2] == 2;
}
// the fused fp32 kernel (k_dgrad32s: all eight parity classes of a 3x3x3 stride-2 conv with a single input in one launch) is
// tried from this many dy voxels on, and under mvd_set_wino_min_items(1) (the tests' "every engine" switch); MVD_DGRAD2=0: off
static const long kDgrad32sMinVoxels = 4096;
static bool dgrad32s_eligible(int N, int D, int H, int W, int C2, const int ks[3], const int st[3]) {
    static const int dg2 = getenv("MVD_DGRAD2") ? atoi(getenv("MVD_DGRAD2")) : 1;
    if (!dg2 || g_engine_mode != 0 || C2 != 0 || !k3s2(ks, st)) return false;
    return (long)N * conv_out_dim(D, 3, 2) * conv_out_dim(H, 3, 2) * conv_out_dim(W, 3, 2) >= kDgrad32sMinVoxels || g_wino_min_items <= 1;
}

/* The general fp32 input gradient; table / table_kind as in mvd_conv3d_fwd_routed (the ub-side table of the weight) */
int mvd_conv3d_dgrad_routed(const float *dy, const float *wb, const float *table, int table_kind, float *dx1, int C1, float *dx2,
                            int C2, int N, int D, int H, int W, int K, const int ksize[3], const int stride[3], void *ws,
                            size_t ws_bytes, void *stream) {
    MVD_REQUIRE(dy && wb && dx1 && C1 > 0 && C2 >= 0 && (C2 == 0 || dx2), "conv3d_dgrad: null pointer / bad channels");
    MVD_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && K > 0, "conv3d_dgrad: bad shape");
    if (check_ks(ksize, stride, "conv3d_dgrad")) return 2;
    MVD_REQUIRE(table_kind >= MVD_CONV_DIRECT && table_kind <= MVD_CONV_WINO2P, "conv3d_dgrad: unknown table kind");
    MVD_REQUIRE(!(table && table_kind == MVD_CONV_WINO2P) || (ksize[0] == 1 && ksize[1] == 3 && ksize[2] == 3),
                "conv3d_dgrad: the in-plane table is that of a 1x3x3 kernel");
    if (dgrad32s_eligible(N, D, H, W, C2, ksize, stride)) {
        int r = dgrad32s(N, D, H, W, C1, K, conv_out_dim(D, 3, 2), conv_out_dim(H, 3, 2), conv_out_dim(W, 3, 2), dy, wb, dx1,
                         as_stream(stream));
        if (r >= 0) return r;
    }
    const WinoTable tab = {table, table_kind, ksize, stride};
    for (int pd = 0; pd < stride[0]; pd++)
        for (int ph = 0; ph < stride[1]; ph++)
            for (int pw = 0; pw < stride[2]; pw++) {
                const int p[3] = {pd, ph, pw};
                FwdGeom g;
                if (!conv_dgrad_class_geom(g, N, D, H, W, C1, C2, K, ksize, stride, p)) continue;
                int r = run_fwd(g, dy, nullptr, wb, nullptr, dx1, dx2, ws, ws_bytes, as_stream(stream), &tab);
                if (r) return r;
            }
    return 0;
}

int mvd_conv3d_dgrad(const float *dy, const float *wb, float *dx1, int C1, float *dx2, int C2, int N, int D, int H, int W,
                     int K, const int ksize[3], const int stride[3], void *ws, size_t ws_bytes, void *stream) {
    return mvd_conv3d_dgrad_routed(dy, wb, nullptr, MVD_CONV_DIRECT, dx1, C1, dx2, C2, N, D, H, W, K, ksize, stride, ws, ws_bytes,
                                   stream);
}

size_t mvd_conv3d_wgrad_workspace_bytes(int C, int K, int T, int N, int Do, int Ho, int Wo) {
    WgradGeom g;
    memset(&g, 0, sizeof(g));
    g.N = N; g.Do = Do; g.Ho = Ho; g.Wo = Wo; g.C1 = C; g.C2 = 0; g.K = K; g.ntaps = g.T = T;
    size_t a = max_sz(wgrad_scalar_ws(g), wgrad_mfma_ws(g));
    return max_sz(a, colsum_ws((long)N * Do * Ho * Wo, K));
}

int mvd_set_wgrad_wino3_min_items(long n) {
    set_wgrad_wino3_min_items(n);
    return 0;
}

int mvd_conv_wgrad_wino3_applicable(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3],
                                    const int stride[3]) {
    if (!conv_args_ok(N, D, H, W, C1, C2, K, ksize, stride, "conv_wgrad_wino3_applicable")) return 0;
    for (int a = 0; a < 3; a++)
        if (ksize[a] != 3 || stride[a] != 1) return 0;
    WgradGeom g;
    conv_wgrad_geom(g, N, D, H, W, C1, C2, K, ksize, stride);
    return wgrad_wino3_selected(g) ? 1 : 0;
}

long mvd_wgrad_wino3_launches(void) { return wgrad_wino3_launches(); }

static_assert(MVD_WG_NONE == WG_NONE && MVD_WG_WINO3 == WG_WINO3 && MVD_WG_WINO2W12 == WG_WINO2W12 && MVD_WG_WINO == WG_WINO &&
                  MVD_WG_SMALLC == WG_SMALLC && MVD_WG_MFMA == WG_MFMA && MVD_WG_WGRAD16 == WG_WGRAD16 &&
                  MVD_WG_WGRAD16Z == WG_WGRAD16Z && MVD_WG_WGRAD16ZS == WG_WGRAD16ZS && MVD_WG_SCALAR == WG_SCALAR,
              "kernel ids of the header and of conv_geom.h");
static_assert(MVD_WGR_F4 == WGR_F4 && MVD_WGR_F16 == WGR_F16 && MVD_WGR_WINO == WGR_WINO && MVD_WGR_WINO2 == WGR_WINO2 &&
                  MVD_WGR_WINO3 == WGR_WINO3 && MVD_WGR_D == WGR_D,
              "reduce ids of the header and of conv_geom.h");
static_assert(MVD_WGB_NONE == WGB_NONE && MVD_WGB_COLSUM == WGB_COLSUM && MVD_WGB_GENERIC == WGB_GENERIC &&
                  MVD_WGB_CONVT == WGB_CONVT && MVD_WGB_SMALLC == WGB_SMALLC && MVD_WGB_WINO3 == WGB_WINO3 &&
                  MVD_WGB_WINO2W12 == WGB_WINO2W12 && MVD_WGB_SLOT28 == WGB_SLOT28 && MVD_WGB_ZMARCH == WGB_ZMARCH,
              "bias-source ids of the header and of conv_geom.h");

int mvd_conv_wgrad_last_kernel(void) { return g_wgrad_last_kernel; }

int mvd_conv_wgrad_plan(int transposed, int is_bf16, int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3],
                        const int stride[3], size_t ws_bytes, int want_bias, int prologue, long *plan) {
    MVD_REQUIRE(plan && stride && (transposed || ksize), "conv_wgrad_plan: null pointer");
    MVD_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && K > 0 && C1 > 0 && C2 >= 0, "conv_wgrad_plan: bad shape");
    MVD_REQUIRE(!transposed || (C2 == 0 && !prologue), "conv_wgrad_plan: a transposed conv has one input and no loader prologue");
    MVD_REQUIRE(!prologue || (is_bf16 && C2 == 0), "conv_wgrad_plan: the loader prologue is bf16 with one input");
    WgradGeom g;
    size_t query;
    if (transposed) {
        for (int a = 0; a < 3; a++) MVD_REQUIRE(stride[a] == 1 || stride[a] == 2, "conv_wgrad_plan: stride must be 1 or 2");
        convT_wgrad_geom(g, N, D, H, W, C1, K, stride);
        query = mvd_convT3d_wgrad_workspace_bytes(C1, K, g.T, N, D, H, W);
    } else {
        if (check_ks(ksize, stride, "conv_wgrad_plan")) return 2;
        conv_wgrad_geom(g, N, D, H, W, C1, C2, K, ksize, stride);
        query = mvd_conv3d_wgrad_workspace_bytes(C1 + C2, K, g.T, N, g.Do, g.Ho, g.Wo);
    }
    if (ws_bytes == 0) ws_bytes = query;
    MVD_REQUIRE(ws_bytes >= query, "conv_wgrad_plan: workspace too small");
    WgradPlan p;
    // the bf16 transposed entry point runs the column sums itself, before the weight gradient
    const bool in_kernel_bias = want_bias && !(transposed && is_bf16);
    const int r = wgrad_plan(g, is_bf16 != 0, ws_bytes, in_kernel_bias, prologue != 0, &p);
    if (r == 3 && prologue) set_error("conv_wgrad_plan: shape not served by the z-marching kernel");
    else if (r == 3) set_error("conv_wgrad_plan: bf16 needs C %% 32 == 0 and K %% 32 == 0 (C=%d+%d K=%d)", C1, C2, K);
    if (r) return 2;
    if (want_bias && !in_kernel_bias) p.bias_src = WGB_COLSUM;
    const long out[MVD_WG_PLAN_LEN] = {p.kernel, p.reduce, p.bias_src, p.TPW, p.NA, p.NB, p.SH, p.TRI, p.TD, p.TH, p.TW,
                                       p.ntd, p.nth, p.ntw, p.ntiles, p.nsplit, p.partials, p.ncb, p.nkb, p.bias_rows,
                                       (long)p.needed_ws, (long)p.ws_bytes, p.wino_mode, p.wino3_on, p.wino3_min_items,
                                       p.bias_fold, p.bf16_kernel, p.engine_mode, p.env_big16, p.env_tri16, p.env_db,
                                       p.env_16z, p.env_16zs, p.env_reduce_g16};
    for (int i = 0; i < MVD_WG_PLAN_LEN; i++) plan[i] = out[i];
    return 0;
}

int mvd_set_wgrad_bias_fold(int on) {
    set_wgrad_bias_fold(on);
    return 0;
}

int mvd_conv3d_wgrad(const float *x1, int C1, const float *x2, int C2, const float *dy, float *dw, float *dbias, int N,
                     int D, int H, int W, int K, const int ksize[3], const int stride[3], void *ws, size_t ws_bytes,
                     void *stream) {
    MVD_REQUIRE(x1 && dy && dw && ws && C1 > 0 && C2 >= 0 && (C2 == 0 || x2), "conv3d_wgrad: null pointer / bad channels");
    MVD_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && K > 0, "conv3d_wgrad: bad shape");
    if (check_ks(ksize, stride, "conv3d_wgrad")) return 2;
    WgradGeom g;
    conv_wgrad_geom(g, N, D, H, W, C1, C2, K, ksize, stride);
    MVD_REQUIRE(ws_bytes >= mvd_conv3d_wgrad_workspace_bytes(C1 + C2, K, g.T, N, g.Do, g.Ho, g.Wo),
                "conv3d_wgrad: workspace too small");
    hipStream_t s = as_stream(stream);
    int dbias_done = 0;
    int r = run_wgrad(g, x1, x2, dy, dw, ws, ws_bytes, s, dbias, &dbias_done);
    if (r) return r;
    if (dbias && !dbias_done) return colsum(dy, dbias, (long)N * g.Do * g.Ho * g.Wo, K, ws, s);  // ws is free again
    return 0;
}

// ------------------------------------------------------------------------------------------------ ConvTranspose3d k == s
int mvd_convT3d_fwd(const float *x, const float *wf, const float *bias, float *y, int N, int D, int H, int W, int C, int K,
                    const int stride[3], void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(x && wf && y && N > 0 && D > 0 && H > 0 && W > 0 && C > 0 && K > 0, "convT3d_fwd: bad arguments");
    for (int a = 0; a < 3; a++) MVD_REQUIRE(stride[a] == 1 || stride[a] == 2, "convT3d_fwd: stride must be 1 or 2");
    if (g_engine_mode == 0 && !g_transp_off) {
        int r = convT_fwd_direct(x, wf, bias, y, N, D, H, W, C, K, stride, as_stream(stream));
        if (r >= 0) return r;
    }
    for (int pd = 0; pd < stride[0]; pd++)
        for (int ph = 0; ph < stride[1]; ph++)
            for (int pw = 0; pw < stride[2]; pw++) {
                const int p[3] = {pd, ph, pw};
                FwdGeom g;
                convT_fwd_class_geom(g, N, D, H, W, C, K, stride, p);
                int r = run_fwd(g, x, nullptr, wf, bias, y, nullptr, ws, ws_bytes, as_stream(stream));
                if (r) return r;
            }
    return 0;
}

int mvd_convT3d_dgrad(const float *dy, const float *wb, float *dx, int N, int D, int H, int W, int C, int K,
                      const int stride[3], void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(dy && wb && dx && N > 0 && D > 0 && H > 0 && W > 0 && C > 0 && K > 0, "convT3d_dgrad: bad arguments");
    for (int a = 0; a < 3; a++) MVD_REQUIRE(stride[a] == 1 || stride[a] == 2, "convT3d_dgrad: stride must be 1 or 2");
    if (g_engine_mode == 0 && !g_transp_off) {
        int r = convT_dgrad_direct(dy, wb, dx, N, D, H, W, C, K, stride, as_stream(stream));
        if (r >= 0) return r;
    }
    FwdGeom g;
    convT_dgrad_geom(g, N, D, H, W, C, K, stride);
    return run_fwd(g, dy, nullptr, wb, nullptr, dx, nullptr, ws, ws_bytes, as_stream(stream));
}

size_t mvd_convT3d_wgrad_workspace_bytes(int C, int K, int T, int N, int D, int H, int W) {
    WgradGeom g;
    memset(&g, 0, sizeof(g));
    g.N = N; g.Do = D; g.Ho = H; g.Wo = W; g.C1 = C; g.K = K; g.ntaps = g.T = T;
    size_t a = max_sz(wgrad_scalar_ws(g), wgrad_mfma_ws(g));
    return max_sz(a, colsum_ws((long)N * D * H * W * T, K));
}

int mvd_convT3d_wgrad(const float *x, const float *dy, float *dw, float *dbias, int N, int D, int H, int W, int C, int K,
                      const int stride[3], void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(x && dy && dw && ws && N > 0 && D > 0 && H > 0 && W > 0 && C > 0 && K > 0, "convT3d_wgrad: bad arguments");
    for (int a = 0; a < 3; a++) MVD_REQUIRE(stride[a] == 1 || stride[a] == 2, "convT3d_wgrad: stride must be 1 or 2");
    WgradGeom g;
    convT_wgrad_geom(g, N, D, H, W, C, K, stride);
    MVD_REQUIRE(ws_bytes >= mvd_convT3d_wgrad_workspace_bytes(C, K, g.T, N, D, H, W), "convT3d_wgrad: workspace too small");
    hipStream_t s = as_stream(stream);
    int dbias_done = 0;  // the MFMA kernel sums the dy fragments it stages where it can (wgrad_mfma)
    int r = run_wgrad(g, x, nullptr, dy, dw, ws, ws_bytes, s, dbias, &dbias_done);
    if (r) return r;
    if (dbias && !dbias_done) return colsum(dy, dbias, (long)N * g.Db * g.Hb * g.Wb, K, ws, s);  // ws is free again
    return 0;
}

// ------------------------------------------------------------------------------------------------ bf16 twins
int mvd_pack_weight_bf16(const float *w, uint16_t *wf, uint16_t *wb, int K, int C, int T, int transposed, void *stream) {
    MVD_REQUIRE(w && (wf || wb) && K > 0 && C > 0 && T > 0 && T <= MVD_MAX_TAPS, "pack_weight_bf16: bad arguments");
    MVD_REQUIRE(!wf || C % 32 == 0, "pack_weight_bf16: wf needs C %% 32 == 0");
    MVD_REQUIRE(!wb || K % 32 == 0, "pack_weight_bf16: wb needs K %% 32 == 0");
    return pack_weight16(w, wf, wb, K, C, T, transposed, as_stream(stream));
}

int mvd_pack_weights_bf16_batch(int n, const float *const *w, uint16_t *const *wf, uint16_t *const *wb, const int *K,
                                const int *C, const int *T, const int *transposed, void *stream) {
    MVD_REQUIRE(n > 0 && w && wf && wb && K && C && T && transposed, "pack_weights_bf16_batch: null table");
    for (int q = 0; q < n; q++) {
        MVD_REQUIRE(w[q] && (wf[q] || wb[q]), "pack_weights_bf16_batch: job without source or destination");
        MVD_REQUIRE(K[q] > 0 && C[q] > 0 && T[q] > 0 && T[q] <= MVD_MAX_TAPS, "pack_weights_bf16_batch: bad K / C / T");
        MVD_REQUIRE(!wf[q] || C[q] % 32 == 0, "pack_weights_bf16_batch: wf needs C %% 32 == 0");
        MVD_REQUIRE(!wb[q] || K[q] % 32 == 0, "pack_weights_bf16_batch: wb needs K %% 32 == 0");
    }
    return pack_weights16_batch(n, w, reinterpret_cast<unsigned short *const *>(wf), reinterpret_cast<unsigned short *const *>(wb),
                                K, C, T, transposed, nullptr, as_stream(stream));
}

int mvd_pack_weights_bf16_batch_pad(int n, const float *const *w, uint16_t *const *wf, uint16_t *const *wb, const int *K,
                                    const int *C, const int *T, const int *transposed, const int *Csrc, void *stream) {
    MVD_REQUIRE(n > 0 && w && wf && wb && K && C && T && transposed && Csrc, "pack_weights_bf16_batch_pad: null table");
    for (int q = 0; q < n; q++) {
        MVD_REQUIRE(w[q] && (wf[q] || wb[q]), "pack_weights_bf16_batch_pad: job without source or destination");
        MVD_REQUIRE(K[q] > 0 && C[q] > 0 && T[q] > 0 && T[q] <= MVD_MAX_TAPS, "pack_weights_bf16_batch_pad: bad K / C / T");
        MVD_REQUIRE(Csrc[q] > 0 && Csrc[q] <= C[q], "pack_weights_bf16_batch_pad: needs 0 < Csrc <= C");
        MVD_REQUIRE(Csrc[q] == C[q] || !transposed[q], "pack_weights_bf16_batch_pad: no padding for transposed-conv weights");
        MVD_REQUIRE(!wf[q] || C[q] % 32 == 0, "pack_weights_bf16_batch_pad: wf needs C %% 32 == 0");
        MVD_REQUIRE(!wb[q] || K[q] % 32 == 0, "pack_weights_bf16_batch_pad: wb needs K %% 32 == 0");
    }
    return pack_weights16_batch(n, w, reinterpret_cast<unsigned short *const *>(wf), reinterpret_cast<unsigned short *const *>(wb),
                                K, C, T, transposed, Csrc, as_stream(stream));
}

int mvd_conv3d_fwd_bf16(const uint16_t *x1, int C1, const uint16_t *x2, int C2, const uint16_t *wf, const float *bias, uint16_t *y, int N,
                   int D, int H, int W, int K, const int ksize[3], const int stride[3], void *ws, size_t ws_bytes,
                   void *stream) {
    MVD_REQUIRE(x1 && wf && y && C1 > 0 && C2 >= 0 && (C2 == 0 || x2), "conv3d_fwd_bf16: null pointer / bad channels");
    MVD_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && K > 0, "conv3d_fwd_bf16: bad shape");
    if (check_ks(ksize, stride, "conv3d_fwd_bf16")) return 2;
    FwdGeom g;
    conv_fwd_geom(g, N, D, H, W, C1, C2, K, ksize, stride);
    return run_fwd16(g, x1, x2, wf, bias, y, nullptr, ws, ws_bytes, as_stream(stream));
}

int mvd_set_bf16_zmarch_kernel(int which) {
    if (which != 0 && which != 1) {
        set_error("set_bf16_zmarch_kernel: 0 = k_fwd16z (32x32x16 tiles), 1 = k_fwd16y (16x16x32 tiles, InstanceNorm fusion)");
        return 2;
    }
    fwd16y_enable(which);
    return 0;
}

int mvd_set_bf16_wgrad_kernel(int which) {
    if (which != 0 && which != 1) {
        set_error("set_bf16_wgrad_kernel: 0 = k_wgrad16 (tiled), 1 = k_wgrad16z (z-marching)");
        return 2;
    }
    wgrad16z_enable(which);
    return 0;
}

int mvd_conv3d_fwd_bf16_stats_tiles(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3],
                                    const int stride[3]) {
    if (!conv_args_ok(N, D, H, W, C1, C2, K, ksize, stride, "conv3d_fwd_bf16_stats_tiles")) return 0;
    FwdGeom g;
    conv_fwd_geom(g, N, D, H, W, C1, C2, K, ksize, stride);
    return fwd_bf16_stats_tiles(g);
}

int mvd_conv3d_fwd_bf16_prologue_ok(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3],
                                    const int stride[3]) {
    if (!conv_args_ok(N, D, H, W, C1, C2, K, ksize, stride, "conv3d_fwd_bf16_prologue_ok")) return 0;
    FwdGeom g;
    conv_fwd_geom(g, N, D, H, W, C1, C2, K, ksize, stride);
    return fwd_bf16_prologue_ok(g);
}

int mvd_conv3d_fwd_bf16_fused(const uint16_t *x1, int C1, const uint16_t *x2, int C2, const uint16_t *wf, const float *bias,
                              uint16_t *y, int N, int D, int H, int W, int K, const int ksize[3], const int stride[3],
                              const float *in_scale, const float *in_shift, float slope, float *tile_stats, int *ntiles_out,
                              void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(x1 && wf && y && C1 > 0 && C2 >= 0 && (C2 == 0 || x2), "conv3d_fwd_bf16_fused: null pointer / bad channels");
    MVD_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && K > 0, "conv3d_fwd_bf16_fused: bad shape");
    MVD_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "conv3d_fwd_bf16_fused: scale and shift come together");
    MVD_REQUIRE(!tile_stats || ntiles_out, "conv3d_fwd_bf16_fused: tile_stats needs ntiles_out");
    if (check_ks(ksize, stride, "conv3d_fwd_bf16_fused")) return 2;
    FwdGeom g;
    conv_fwd_geom(g, N, D, H, W, C1, C2, K, ksize, stride);
    Fwd16Fuse f;
    f.tile_stats = tile_stats;
    f.ntiles = ntiles_out;
    f.in_scale = in_scale;
    f.in_shift = in_shift;
    f.slope = slope;
    if (ntiles_out) *ntiles_out = 0;
    return run_fwd16(g, x1, x2, wf, bias, y, nullptr, ws, ws_bytes, as_stream(stream), &f);
}

// the fused bf16 kernel (k_dgrad16s) is tried from this many dy voxels on
static const long kDgrad16sMinVoxels = 512;
static int dgrad_bf16_impl(const uint16_t *dy, const uint16_t *wb, uint16_t *dx1, int C1, uint16_t *dx2, int C2, int N, int D, int H,
                           int W, int K, const int ksize[3], const int stride[3], void *ws, size_t ws_bytes, void *stream,
                           int acc) {
    MVD_REQUIRE(dy && wb && dx1 && C1 > 0 && C2 >= 0 && (C2 == 0 || dx2), "conv3d_dgrad_bf16: null pointer / bad channels");
    MVD_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && K > 0, "conv3d_dgrad_bf16: bad shape");
    if (check_ks(ksize, stride, "conv3d_dgrad_bf16")) return 2;
    // 3x3x3 stride-2 conv with 32-multiple channels and a single input: all eight parity classes in one kernel
    const int od[3] = {conv_out_dim(D, ksize[0], stride[0]), conv_out_dim(H, ksize[1], stride[1]), conv_out_dim(W, ksize[2], stride[2])};
    if (g_engine_mode == 0 && C2 == 0 && k3s2(ksize, stride) && (long)N * od[0] * od[1] * od[2] >= kDgrad16sMinVoxels) {
        int r = dgrad16s(N, D, H, W, C1, K, od[0], od[1], od[2], dy, wb, dx1, as_stream(stream), acc);
        if (r >= 0) return r;
    }
    // one launch per output-parity class (1 class per stride-1 axis, 2 per stride-2 axis)
    for (int pd = 0; pd < stride[0]; pd++)
        for (int ph = 0; ph < stride[1]; ph++)
            for (int pw = 0; pw < stride[2]; pw++) {
                const int p[3] = {pd, ph, pw};
                FwdGeom g;
                if (!conv_dgrad_class_geom(g, N, D, H, W, C1, C2, K, ksize, stride, p)) continue;
                g.acc = (int8_t)acc;
                int r = run_fwd16(g, dy, nullptr, wb, nullptr, dx1, dx2, ws, ws_bytes, as_stream(stream));
                if (r) return r;
            }
    return 0;
}

int mvd_conv3d_dgrad_bf16(const uint16_t *dy, const uint16_t *wb, uint16_t *dx1, int C1, uint16_t *dx2, int C2, int N, int D, int H, int W,
                     int K, const int ksize[3], const int stride[3], void *ws, size_t ws_bytes, void *stream) {
    return dgrad_bf16_impl(dy, wb, dx1, C1, dx2, C2, N, D, H, W, K, ksize, stride, ws, ws_bytes, stream, 0);
}

static bool strided3(const int ksize[3], const int stride[3]) {
    return ksize[0] == 3 && ksize[1] == 3 && ksize[2] == 3 && (stride[0] == 2 || stride[1] == 2 || stride[2] == 2);
}

int mvd_conv3d_dgrad_acc_ok(int is_bf16, int N, int D, int H, int W, int C1, int K, const int ksize[3], const int stride[3]) {
    if (!conv_args_ok(N, D, H, W, C1, 0, K, ksize, stride, "conv3d_dgrad_acc_ok")) return 0;
    if (C1 % 32 || K % 32 || g_engine_mode != 0) return 0;
    if (is_bf16) return strided3(ksize, stride) ? 1 : 0;   // every parity class runs on the generic bf16 kernel
    // fp32: the fused stride-2 kernel, and only with a dy sample below 2^31 bytes (a condition of this accumulating path alone)
    return (dgrad32s_eligible(N, D, H, W, 0, ksize, stride) &&
            (long)conv_out_dim(D, 3, 2) * conv_out_dim(H, 3, 2) * conv_out_dim(W, 3, 2) * K * 4 < (1L << 31)) ? 1 : 0;
}

int mvd_conv3d_dgrad_bf16_acc(const uint16_t *dy, const uint16_t *wb, uint16_t *dx1, int C1, int N, int D, int H, int W, int K,
                              const int ksize[3], const int stride[3], void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(mvd_conv3d_dgrad_acc_ok(1, N, D, H, W, C1, K, ksize, stride), "conv3d_dgrad_bf16_acc: no accumulating kernel for this "
                "shape (ask mvd_conv3d_dgrad_acc_ok first)");
    return dgrad_bf16_impl(dy, wb, dx1, C1, nullptr, 0, N, D, H, W, K, ksize, stride, ws, ws_bytes, stream, 1);
}

int mvd_conv3d_dgrad_acc(const float *dy, const float *wb, float *dx1, int C1, int N, int D, int H, int W, int K,
                         const int ksize[3], const int stride[3], void *stream) {
    MVD_REQUIRE(dy && wb && dx1, "conv3d_dgrad_acc: null pointer");
    MVD_REQUIRE(mvd_conv3d_dgrad_acc_ok(0, N, D, H, W, C1, K, ksize, stride), "conv3d_dgrad_acc: no accumulating kernel for this shape "
                "(ask mvd_conv3d_dgrad_acc_ok first)");
    int r = dgrad32s(N, D, H, W, C1, K, conv_out_dim(D, 3, 2), conv_out_dim(H, 3, 2), conv_out_dim(W, 3, 2), dy, wb, dx1, as_stream(stream), 1);
    if (r < 0) {
        set_error("conv3d_dgrad_acc: the fused stride-2 kernel refused the shape");
        return 3;
    }
    return r;
}

int mvd_convT3d_fwd_bf16(const uint16_t *x, const uint16_t *wf, const float *bias, uint16_t *y, int N, int D, int H, int W, int C, int K,
                    const int stride[3], void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(x && wf && y && N > 0 && D > 0 && H > 0 && W > 0 && C > 0 && K > 0, "convT3d_fwd_bf16: bad arguments");
    for (int a = 0; a < 3; a++) MVD_REQUIRE(stride[a] == 1 || stride[a] == 2, "convT3d_fwd_bf16: stride must be 1 or 2");
    if (!g_transp_off) {
        int r = convT_fwd_direct16(x, wf, bias, y, N, D, H, W, C, K, stride, as_stream(stream));
        if (r >= 0) return r;
    }
    for (int pd = 0; pd < stride[0]; pd++)
        for (int ph = 0; ph < stride[1]; ph++)
            for (int pw = 0; pw < stride[2]; pw++) {
                const int p[3] = {pd, ph, pw};
                FwdGeom g;
                convT_fwd_class_geom(g, N, D, H, W, C, K, stride, p);
                int r = run_fwd16(g, x, nullptr, wf, bias, y, nullptr, ws, ws_bytes, as_stream(stream));
                if (r) return r;
            }
    return 0;
}

int mvd_convT3d_dgrad_bf16(const uint16_t *dy, const uint16_t *wb, uint16_t *dx, int N, int D, int H, int W, int C, int K,
                      const int stride[3], void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(dy && wb && dx && N > 0 && D > 0 && H > 0 && W > 0 && C > 0 && K > 0, "convT3d_dgrad_bf16: bad arguments");
    for (int a = 0; a < 3; a++) MVD_REQUIRE(stride[a] == 1 || stride[a] == 2, "convT3d_dgrad_bf16: stride must be 1 or 2");
    if (!g_transp_off) {
        int r = convT_dgrad_direct16(dy, wb, dx, N, D, H, W, C, K, stride, as_stream(stream));
        if (r >= 0) return r;
    }
    FwdGeom g;
    convT_dgrad_geom(g, N, D, H, W, C, K, stride);
    return run_fwd16(g, dy, nullptr, wb, nullptr, dx, nullptr, ws, ws_bytes, as_stream(stream));
}

int mvd_conv3d_wgrad_bf16(const uint16_t *x1, int C1, const uint16_t *x2, int C2, const uint16_t *dy, float *dw, float *dbias, int N,
                     int D, int H, int W, int K, const int ksize[3], const int stride[3], void *ws, size_t ws_bytes,
                     void *stream) {
    MVD_REQUIRE(x1 && dy && dw && ws && C1 > 0 && C2 >= 0 && (C2 == 0 || x2), "conv3d_wgrad_bf16: null pointer / bad channels");
    MVD_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && K > 0, "conv3d_wgrad_bf16: bad shape");
    if (check_ks(ksize, stride, "conv3d_wgrad_bf16")) return 2;
    WgradGeom g;
    conv_wgrad_geom(g, N, D, H, W, C1, C2, K, ksize, stride);
    MVD_REQUIRE(ws_bytes >= mvd_conv3d_wgrad_workspace_bytes(C1 + C2, K, g.T, N, g.Do, g.Ho, g.Wo),
                "conv3d_wgrad_bf16: workspace too small");
    hipStream_t s = as_stream(stream);
    // the 27-tap kernel produces the bias gradient from its idle tap slot; the other shapes take the column-sum pass
    int dbias_done = 0;
    int r = run_wgrad16(g, x1, x2, dy, dw, ws, ws_bytes, s, dbias, &dbias_done);
    if (r) return r;
    if (dbias && !dbias_done) return colsum(reinterpret_cast<const float *>(dy), dbias, (long)N * g.Do * g.Ho * g.Wo, K, ws, s, true);
    return 0;
}

int mvd_conv3d_wgrad_bf16_prologue_ok(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3], const int stride[3]) {
    if (!conv_args_ok(N, D, H, W, C1, C2, K, ksize, stride, "conv3d_wgrad_bf16_prologue_ok")) return 0;
    WgradGeom g;
    conv_wgrad_geom(g, N, D, H, W, C1, C2, K, ksize, stride);
    return wgrad16z_prologue_ok(g) ? 1 : 0;
}

int mvd_conv3d_wgrad_bf16_fused(const uint16_t *x1, int C1, const uint16_t *dy, float *dw, float *dbias, int N, int D, int H, int W,
                                int K, const int ksize[3], const int stride[3], const float *in_scale, const float *in_shift,
                                float slope, void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(x1 && dy && dw && ws && in_scale && in_shift && C1 > 0, "conv3d_wgrad_bf16_fused: null pointer / bad channels");
    MVD_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && K > 0, "conv3d_wgrad_bf16_fused: bad shape");
    if (check_ks(ksize, stride, "conv3d_wgrad_bf16_fused")) return 2;
    WgradGeom g;
    conv_wgrad_geom(g, N, D, H, W, C1, 0, K, ksize, stride);
    MVD_REQUIRE(wgrad16z_prologue_ok(g), "conv3d_wgrad_bf16_fused: shape not served by the z-marching kernel (query _prologue_ok)");
    MVD_REQUIRE(ws_bytes >= mvd_conv3d_wgrad_workspace_bytes(C1, K, g.T, N, g.Do, g.Ho, g.Wo),
                "conv3d_wgrad_bf16_fused: workspace too small");
    hipStream_t s = as_stream(stream);
    int dbias_done = 0;
    WgradPlan p;
    if (wgrad_plan(g, true, ws_bytes, dbias != nullptr, true, &p)) {
        set_error("conv3d_wgrad_bf16_fused: the z-marching kernel refused the launch (workspace?)");
        return 2;
    }
    const int r = wgrad_launch(p, g, reinterpret_cast<const float *>(x1), nullptr, reinterpret_cast<const float *>(dy), dw, ws, s,
                               dbias, &dbias_done, in_scale, in_shift, slope);
    if (r) return r;
    if (dbias && !dbias_done) return colsum(reinterpret_cast<const float *>(dy), dbias, (long)N * g.Do * g.Ho * g.Wo, K, ws, s, true);
    return 0;
}

int mvd_convT3d_wgrad_bf16(const uint16_t *x, const uint16_t *dy, float *dw, float *dbias, int N, int D, int H, int W, int C, int K,
                      const int stride[3], void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(x && dy && dw && ws && N > 0 && D > 0 && H > 0 && W > 0 && C > 0 && K > 0, "convT3d_wgrad_bf16: bad arguments");
    for (int a = 0; a < 3; a++) MVD_REQUIRE(stride[a] == 1 || stride[a] == 2, "convT3d_wgrad_bf16: stride must be 1 or 2");
    WgradGeom g;
    convT_wgrad_geom(g, N, D, H, W, C, K, stride);
    MVD_REQUIRE(ws_bytes >= mvd_convT3d_wgrad_workspace_bytes(C, K, g.T, N, D, H, W), "convT3d_wgrad_bf16: workspace too small");
    hipStream_t s = as_stream(stream);
    if (dbias) {
        int r = colsum(reinterpret_cast<const float *>(dy), dbias, (long)N * g.Db * g.Hb * g.Wb, K, ws, s, true);
        if (r) return r;
    }
    return run_wgrad16(g, x, nullptr, dy, dw, ws, ws_bytes, s);
}
}
