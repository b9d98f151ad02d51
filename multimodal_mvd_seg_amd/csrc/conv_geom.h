// Generic "gathered-tap GEMM" problem descriptors shared by the scalar and the MFMA conv engines.
//
// Forward-type problem (conv fwd, conv dgrad, convT fwd, convT dgrad all reduce to it):
//   Y[n, o*so + oo, k] = bias[k] + sum_{t < ntaps} sum_{c < C1+C2} A[n, o*sa + off[t], c] * W[wt[t]][c][k]
// with o over the iteration grid (Do,Ho,Wo), A = channel concat of a1 [.,C1] and a2 [.,C2] with spatial dims
// (Di,Hi,Wi) (reads outside are zero), Y = channel split into y1 [.,K1] and y2 [.,K2] with spatial dims (Dy,Hy,Wy).
//
// Wgrad-type problem (conv wgrad, convT wgrad):
//   dW[wt[t]][c][k] = sum_n sum_o A[n, o*sa + off[t], c] * B[n, o*sb + ob[t], k]
// B [.,K] with spatial dims (Db,Hb,Wb) (reads outside are zero).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace mvd {

// Packed weight layout shared by mvd_pack_weight, the scalar engine and the MFMA engine.  For a reduce dimension
// C (multiple of 4) the tensor is stored in chunks of CK = 8 (or 4) reduce-channels, each chunk tap-major, and inside
// a (chunk, tap) as [h][k][e] with c = cc*CK + h*(CK/2) + e: exactly the image one workgroup stages into LDS and
// the order the 32x32x2 fp32 MFMA consumes (lane half h takes CK/2 consecutive k-steps from one ds_read_b128/b64).
// C % 4 != 0 falls back to plain [t][c][k] (scalar engine only).
// CK = 32 whenever possible: a 32-channel chunk of an NDHWC voxel is one whole 128-byte line, so the staging pass of
// the MFMA kernels touches every input line exactly once (8-channel chunks re-fetched each line 4 times from HBM).
__host__ __device__ inline int wl_ck(int C) {
    return (C % 32 == 0) ? 32 : ((C % 8 == 0) ? 8 : ((C % 4 == 0) ? 4 : 0));
}
__host__ __device__ inline size_t widx(int CK, int T, int C, int K, int t, int c, int k) {
    if (CK == 0) return ((size_t)t * C + c) * K + k;
    const int hh = CK / 2;
    const int cc = c / CK, r = c % CK;
    return ((((size_t)cc * T + t) * 2 + r / hh) * K + k) * hh + (r % hh);
}

struct FwdGeom {
    int N;
    int T;  // taps of the full weight tensor (packed-layout stride)
    int Di, Hi, Wi;
    int Do, Ho, Wo;
    int Dy, Hy, Wy;
    int C1, C2, K1, K2;
    int ntaps;
    int sa[3], so[3], oo[3];
    int8_t off[27][3];
    int8_t wt[27];
    int8_t acc;  // 1: y1 += result (the gradient of a tensor with a second consumer, ops._GradShare); engines that support it:
                 // k_fwd16 / k_split_reduce16 (bf16 generic), k_dgrad32s (fp32); the others refuse (-1)
};

struct WgradGeom {
    int N;
    int Di, Hi, Wi;  // A dims
    int Db, Hb, Wb;  // B dims
    int Do, Ho, Wo;  // iteration grid
    int C1, C2, K;
    int ntaps;       // taps of this launch
    int T;           // taps of the full weight tensor (layout stride)
    int sa[3], sb[3];
    int8_t off[27][3], ob[27][3];
    int8_t wt[27];
    int transposed_out;  // 0: dw[k][c][T] (Conv3d), 1: dw[c][k][T] (ConvTranspose3d)
};

// ------------------------------------------------------------------------------------------------ geometry builders
// The one place each descriptor is built: the fp32 and the bf16 entry points of conv.hip call the same builder
// (tests/host/conv_geom_dump.cpp prints their bytes, tests/golden/conv_geom.txt pins them).  Kernel sizes are 1 or 3 and
// strides 1 or 2 per axis (check_ks at the entry points); every builder clears the struct first, padding included.
inline int conv_out_dim(int in, int k, int s) { return (in + 2 * ((k - 1) / 2) - k) / s + 1; }

// every tap of a ks[0] x ks[1] x ks[2] kernel in raster order, offsets relative to the centre; returns their number
inline int conv_full_taps(const int ks[3], int8_t off[27][3], int8_t wt[27]) {
    int t = 0;
    for (int a = 0; a < ks[0]; a++)
        for (int b = 0; b < ks[1]; b++)
            for (int c = 0; c < ks[2]; c++) {
                off[t][0] = a - (ks[0] - 1) / 2;
                off[t][1] = b - (ks[1] - 1) / 2;
                off[t][2] = c - (ks[2] - 1) / 2;
                wt[t] = t;
                t++;
            }
    return t;
}

inline void conv_fwd_geom(FwdGeom &g, int N, int D, int H, int W, int C1, int C2, int K, const int ks[3], const int st[3]) {
    memset(&g, 0, sizeof(g));
    g.N = N;
    g.Di = D; g.Hi = H; g.Wi = W;
    g.Do = conv_out_dim(D, ks[0], st[0]); g.Ho = conv_out_dim(H, ks[1], st[1]); g.Wo = conv_out_dim(W, ks[2], st[2]);
    g.Dy = g.Do; g.Hy = g.Ho; g.Wy = g.Wo;
    g.C1 = C1; g.C2 = C2; g.K1 = K; g.K2 = 0;
    g.ntaps = g.T = conv_full_taps(ks, g.off, g.wt);
    for (int a = 0; a < 3; a++) {
        g.sa[a] = st[a];
        g.so[a] = 1;
        g.oo[a] = 0;
    }
}

inline void conv_wgrad_geom(WgradGeom &g, int N, int D, int H, int W, int C1, int C2, int K, const int ks[3], const int st[3]) {
    memset(&g, 0, sizeof(g));
    g.N = N;
    g.Di = D; g.Hi = H; g.Wi = W;
    g.Do = conv_out_dim(D, ks[0], st[0]); g.Ho = conv_out_dim(H, ks[1], st[1]); g.Wo = conv_out_dim(W, ks[2], st[2]);
    g.Db = g.Do; g.Hb = g.Ho; g.Wb = g.Wo;
    g.C1 = C1; g.C2 = C2; g.K = K;
    g.ntaps = g.T = conv_full_taps(ks, g.off, g.wt);
    for (int a = 0; a < 3; a++) {
        g.sa[a] = st[a];
        g.sb[a] = 1;
    }
    g.transposed_out = 0;
}

// Input gradient of the conv [N,D,H,W,C1+C2] -> K as forward-type problems: one per output-parity class p (1 class per
// stride-1 axis, 2 per stride-2 axis), reading dy and writing the voxels o*st + p of dx1 / dx2.  false: the class has no
// voxel or no tap (nothing to launch; g is then unspecified).  g.acc stays 0.
inline bool conv_dgrad_class_geom(FwdGeom &g, int N, int D, int H, int W, int C1, int C2, int K, const int ks[3],
                                  const int st[3], const int p[3]) {
    const int dims[3] = {D, H, W};
    memset(&g, 0, sizeof(g));
    g.N = N;
    g.Di = conv_out_dim(D, ks[0], st[0]); g.Hi = conv_out_dim(H, ks[1], st[1]); g.Wi = conv_out_dim(W, ks[2], st[2]);
    g.Dy = D; g.Hy = H; g.Wy = W;
    int grid[3];
    for (int a = 0; a < 3; a++) {
        grid[a] = (dims[a] - p[a] + st[a] - 1) / st[a];
        if (grid[a] <= 0) return false;
        g.sa[a] = 1;
        g.so[a] = st[a];
        g.oo[a] = p[a];
    }
    g.Do = grid[0]; g.Ho = grid[1]; g.Wo = grid[2];
    g.C1 = K; g.C2 = 0; g.K1 = C1; g.K2 = C2;
    int nt = 0;
    for (int ta = 0; ta < ks[0]; ta++)
        for (int tb = 0; tb < ks[1]; tb++)
            for (int tc = 0; tc < ks[2]; tc++) {
                const int t3[3] = {ta, tb, tc};
                int off[3];
                bool ok = true;
                for (int a = 0; a < 3; a++) {
                    int num = p[a] + (ks[a] - 1) / 2 - t3[a];  // dy index q: q*s + t - pad = o*s + p
                    if (num % st[a] != 0) { ok = false; break; }
                    off[a] = num / st[a];
                }
                if (!ok) continue;
                for (int a = 0; a < 3; a++) g.off[nt][a] = (int8_t)off[a];
                g.wt[nt] = (int8_t)((ta * ks[1] + tb) * ks[2] + tc);
                nt++;
            }
    g.ntaps = nt;
    g.T = ks[0] * ks[1] * ks[2];
    return nt > 0;
}

// ConvTranspose3d with kernel == stride, x [N,D,H,W,C] -> y [N,D*st,...,K]: the forward is one single-tap problem per
// output-parity class p ...
inline void convT_fwd_class_geom(FwdGeom &g, int N, int D, int H, int W, int C, int K, const int st[3], const int p[3]) {
    memset(&g, 0, sizeof(g));
    g.N = N;
    g.Di = g.Do = D; g.Hi = g.Ho = H; g.Wi = g.Wo = W;
    g.Dy = D * st[0]; g.Hy = H * st[1]; g.Wy = W * st[2];
    g.C1 = C; g.K1 = K;
    g.ntaps = 1;
    g.T = st[0] * st[1] * st[2];
    g.wt[0] = (int8_t)((p[0] * st[1] + p[1]) * st[2] + p[2]);
    for (int a = 0; a < 3; a++) {
        g.sa[a] = 1;
        g.so[a] = st[a];
        g.oo[a] = p[a];
    }
}

// ... its input gradient one strided problem over all the taps ...
inline void convT_dgrad_geom(FwdGeom &g, int N, int D, int H, int W, int C, int K, const int st[3]) {
    memset(&g, 0, sizeof(g));
    g.N = N;
    g.Di = D * st[0]; g.Hi = H * st[1]; g.Wi = W * st[2];
    g.Do = g.Dy = D; g.Ho = g.Hy = H; g.Wo = g.Wy = W;
    g.C1 = K; g.K1 = C;
    int t = 0;
    for (int pd = 0; pd < st[0]; pd++)
        for (int ph = 0; ph < st[1]; ph++)
            for (int pw = 0; pw < st[2]; pw++) {
                g.off[t][0] = pd; g.off[t][1] = ph; g.off[t][2] = pw;
                g.wt[t] = t;
                t++;
            }
    g.ntaps = g.T = t;
    for (int a = 0; a < 3; a++) {
        g.sa[a] = st[a];
        g.so[a] = 1;
        g.oo[a] = 0;
    }
}

// ... and its weight gradient
inline void convT_wgrad_geom(WgradGeom &g, int N, int D, int H, int W, int C, int K, const int st[3]) {
    memset(&g, 0, sizeof(g));
    g.N = N;
    g.Di = g.Do = D; g.Hi = g.Ho = H; g.Wi = g.Wo = W;
    g.Db = D * st[0]; g.Hb = H * st[1]; g.Wb = W * st[2];
    g.C1 = C; g.C2 = 0; g.K = K;
    int t = 0;
    for (int pd = 0; pd < st[0]; pd++)
        for (int ph = 0; ph < st[1]; ph++)
            for (int pw = 0; pw < st[2]; pw++) {
                g.ob[t][0] = pd; g.ob[t][1] = ph; g.ob[t][2] = pw;
                g.wt[t] = t;
                t++;
            }
    g.ntaps = g.T = t;
    for (int a = 0; a < 3; a++) {
        g.sa[a] = 1;
        g.sb[a] = st[a];
    }
    g.transposed_out = 1;
}

// ------------------------------------------------------------------------------------------------ tile walk (k_wgrad_wino3)
// A split of k_wgrad_wino3 visits the tiles split, split + nsplit, ...; tile = ((n * ntd + td) * nth + th) * ntw + tw.
// The walk keeps (tw, th, td, n) and adds the host-computed digits of nsplit with carries instead of dividing the tile
// index again for every tile: a digit is below its extent, so a sum with a carry is below twice the extent and one
// conditional subtraction per digit is enough.  n is not bounded: past the last tile it only says "no tile".
// tests/host/wgrad_walk_main.cpp checks the walk against plain division.
struct TileWalk {
    int tw, th, td, n;
};
__host__ __device__ inline TileWalk tile_walk_at(int tile, int ntw, int nth, int ntd) {
    TileWalk p;
    unsigned r = (unsigned)tile;
    p.tw = (int)(r % (unsigned)ntw); r /= (unsigned)ntw;
    p.th = (int)(r % (unsigned)nth); r /= (unsigned)nth;
    p.td = (int)(r % (unsigned)ntd);
    p.n = (int)(r / (unsigned)ntd);
    return p;
}
__host__ __device__ inline void tile_walk_advance(TileWalk &p, const TileWalk &d, int ntw, int nth, int ntd) {
    int v = p.tw + d.tw, c = v >= ntw;
    p.tw = c ? v - ntw : v;
    v = p.th + d.th + c; c = v >= nth;
    p.th = c ? v - nth : v;
    v = p.td + d.td + c; c = v >= ntd;
    p.td = c ? v - ntd : v;
    p.n += d.n + c;
}

// ------------------------------------------------------------------------------------------------ weight-gradient plan
// The tile descriptors the weight-gradient kernels take by value (k_wgrad_mfma / k_wgrad16 / k_wgrad_smallc / k_wgrad_wino*:
// WgTile; k_wgrad16z / k_wgrad16zs: WgZTile; k_wgrad_wino3: Wg3Tile) and the plan that fills them.
struct WgTile {
    int TD, TH, TW, lTH, lTW;
    int EAh, EAw, nslotsA, minA[3];
    int EBh, EBw, nslotsB, minB[3];
    int magAw, magAhw, magBw, magBhw;  // 16-bit reciprocal multipliers: q = (n * mag) >> 16 (exact, host-verified)
    int ntd, nth, ntw, nsplit, nkb;
    int ntiles;
    int toffA[27], toffB[27];
    int dbg;
};
struct WgZTile {
    int nty, ntx, nzc, zc;   // column tiles, z chunks per column, planes per chunk
    int nunits, nsplit, nkb;
};
struct Wg3Tile {
    int ntd, nth, ntw;  // 2 x 8 x 8 tiles along D, H, W
    int ntiles, nsplit, nkb;
    TileWalk step;  // tile_walk_at(nsplit): what a split adds per tile
};

// kernel / reduce / bias-source ids: MVD_WG_*, MVD_WGR_*, MVD_WGB_* of include/mvdseg_hip.h (conv.hip checks they agree)
enum { WG_NONE = 0, WG_WINO3, WG_WINO2W12, WG_WINO, WG_SMALLC, WG_MFMA, WG_WGRAD16, WG_WGRAD16Z, WG_WGRAD16ZS, WG_SCALAR };
enum { WGR_NONE = 0, WGR_F4, WGR_F16, WGR_WINO, WGR_WINO2, WGR_WINO3, WGR_D };
enum { WGB_NONE = 0, WGB_COLSUM, WGB_GENERIC, WGB_CONVT, WGB_SMALLC, WGB_WINO3, WGB_WINO2W12, WGB_SLOT28, WGB_ZMARCH };

// What one weight-gradient call runs: filled by wgrad_plan (conv_mfma.hip; host arithmetic only, no device call, no
// pointer) and consumed by the launch code -- wgrad_launch launches plan.kernel with plan.tg / tz / t3 and nothing else.
// The z-marching kernels report their column tile as (TD, TH, TW) = (zc, 8 or 4, 32), (ntd, nth, ntw) = (nzc, nty, ntx)
// and their units as ntiles.
struct WgradPlan {
    int kernel, reduce, bias_src;
    int TPW, NA, NB, SH, TRI;
    int TD, TH, TW, ntd, nth, ntw;
    long ntiles;
    int nsplit, partials;       // split-K workgroups along grid x; partial tensors each of them writes (2: k_wgrad_mfma)
    int ncb, nkb;
    int bias_rows;              // rows [K] behind the partials that the reduce sums into dbias (0: none)
    size_t bias_off;            // their byte offset in the workspace
    size_t needed_ws, ws_bytes; // bytes the chosen path touches; the workspace the plan was made for
    int cfg, pro;               // tile configuration of the tiled kernels; the loader prologue of k_wgrad16z
    long chunk;                 // k_wgrad_scalar: voxels per split
    // the switches it read
    int wino_mode, wino3_on, bias_fold, bf16_kernel, engine_mode;
    long wino3_min_items;
    int env_big16, env_tri16, env_db, env_16z, env_16zs, env_reduce_g16;
    WgTile tg;
    WgZTile tz;
    Wg3Tile t3;
};
// 0: planned; 1: an error (message set: a workspace below what the tiled kernels need); 3: bf16 and no kernel takes the shape
int wgrad_plan(const WgradGeom &g, bool bf16_in, size_t ws_bytes, bool want_bias, bool prologue, WgradPlan *plan);
// k_wgrad_scalar whatever the shape (fp32 operands that are not 16-byte aligned)
void wgrad_plan_scalar(const WgradGeom &g, size_t ws_bytes, bool want_bias, WgradPlan *plan);
// launches what the plan says (fp32 operands for bf16_in == false, bf16 bits behind the same pointers otherwise)
int wgrad_launch(const WgradPlan &p, const WgradGeom &g, const float *a1, const float *a2, const float *b, float *dw, void *ws,
                 hipStream_t s, float *dbias, int *dbias_done, const float *in_scale = nullptr, const float *in_shift = nullptr,
                 float slope = 0.f);
extern int g_wgrad_last_kernel;  // plan.kernel of the most recent launch (one host store beside each hipLaunchKernelGGL)
// the per-file halves of the plan and of the launch
int conv_engine_mode();                                     // conv.hip: 0 auto, 1 scalar only
int wgrad_scalar_split(const WgradGeom &g, long *chunk);    // conv.hip
bool wgrad16z_plan(const WgradGeom &g, bool pro, bool want_bias, size_t ws_bytes, WgradPlan *p);   // conv_bf16w.hip
bool wgrad16zs_plan(const WgradGeom &g, size_t ws_bytes, WgradPlan *p);
int wgrad16z_launch(const WgradPlan &p, const WgradGeom &g, const unsigned short *a1, const unsigned short *a2,
                    const unsigned short *b, void *ws, hipStream_t s, const float *in_scale, const float *in_shift, float slope);
int wgrad16zs_launch(const WgradPlan &p, const WgradGeom &g, const unsigned short *a1, const unsigned short *b, void *ws,
                     hipStream_t s);
int wgrad16z_mode_now();
int wgrad16z_env();
int wgrad16zs_env();
bool wgrad_wino3_plan(const WgradGeom &g, int nsplit, bool want_bias, size_t ws_bytes, WgradPlan *p);  // conv_wgrad_wino3.hip
int wgrad_wino3_launch(const WgradPlan &p, const WgradGeom &g, const float *a1, const float *a2, const float *b, float *dw,
                       void *ws, hipStream_t s, float *dbias, int *dbias_done);
long wgrad_wino3_min_items();

// engines (return 0 ok, >0 error, -1 = shape not supported by this engine)
int fwd_scalar(const FwdGeom &g, const float *a1, const float *a2, const float *w, const float *bias, float *y1,
               float *y2, hipStream_t s);
// ws/ws_bytes: optional scratch for the split-reduce path of skinny problems (few tiles, many reduce channels)
size_t fwd_mfma_ws(int N, long out_vox, int K);
// stats (optional, [N][stats_tiles][K][2]) / stats_done: the InstanceNorm statistics epilogue of the chunked and the stride-2
// kernels (per-wave tiles of at most 64 values; plain forward convs); it runs when stats_tiles is the kernel's own count.
// plan (optional): nothing is launched, *plan = that count for the kernel that would run (0: no epilogue)
int fwd_mfma(const FwdGeom &g, const float *a1, const float *a2, const float *w, const float *bias, float *y1, float *y2,
             void *ws, size_t ws_bytes, hipStream_t s, float *stats = nullptr, long stats_tiles = 0, int *stats_done = nullptr,
             long *plan = nullptr);
size_t wgrad_scalar_ws(const WgradGeom &g);
int wgrad_scalar(const WgradPlan &p, const WgradGeom &g, const float *a1, const float *a2, const float *b, float *dw, void *ws,
                 hipStream_t s);
size_t wgrad_mfma_ws(const WgradGeom &g);

// fp32 Winograd F(2,3)-along-W engine for plain 3x3x3 stride-1 problems (conv_wino.hip); u = Winograd-domain weights
// stats / stats_done (optional): the F(2x2,3x3) kernel can also emit per-tile (sum y, sum y^2) per output channel,
// [n][tile][K][2] floats with tile = 4x4x8-voxel tiles in raster order (the InstanceNorm statistics epilogue)
int fwd_wino(const FwdGeom &g, const float *a1, const float *a2, const float *u, const float *bias, float *y1, float *y2,
             hipStream_t s, float *stats = nullptr, int *stats_done = nullptr);
int pack_weight_wino(const float *w, float *uf, float *ub, int K, int C, hipStream_t s);
// F(2x2x2,3x3x3) engine (conv_wino3.hip): same contract as fwd_wino with the 3-D table of pack_weight_wino3
// (64*C*K floats); the statistics come out in the same 4x4x8-tile layout
int fwd_wino3(const FwdGeom &g, const float *a1, const float *a2, const float *u, const float *bias, float *y1, float *y2,
              hipStream_t s, float *stats = nullptr, int *stats_done = nullptr);
int pack_weight_wino3(const float *w, float *uf, float *ub, int K, int C, hipStream_t s);
int wino3_enabled();  // MVD_WINO3: 0 off, 1 (default) on
// F(2x2,3x3) engine of the 9-tap in-plane (1x3x3, stride 1) problems (conv_wino2p.hip): the fwd_wino contract with the
// table of pack_weight_wino2p (16*C*K floats); no statistics epilogue.  wino2p_items: its work items (4 planes x 4 x 8
// outputs x 32 channels) for N*D planes
int fwd_wino2p(const FwdGeom &g, const float *a1, const float *a2, const float *u, const float *bias, float *y1, float *y2,
               hipStream_t s);
int pack_weight_wino2p(const float *w, float *uf, float *ub, int K, int C, hipStream_t s);
long wino2p_items(int N, int D, int H, int W, int K);
int dgrad32s(int N, int D, int H, int W, int C, int K, int Do, int Ho, int Wo, const float *dy, const float *wb, float *dx,
             hipStream_t s, int accumulate = 0);
// bf16 twin (conv_bf16.hip): all eight parity classes of a 3x3x3 stride-2 conv's input gradient from one staged dy tile
int dgrad16s(int N, int D, int H, int W, int C, int K, int Do, int Ho, int Wo, const unsigned short *dy, const unsigned short *wb,
             unsigned short *dx, hipStream_t s, int accumulate = 0);
// bf16 z-marching stride-2 forward conv 32 -> 64 channels (conv_bf16s.hip): -1 = not this kernel's shape
int launch_fwd16ys(const FwdGeom &g, const unsigned short *a1, const unsigned short *a2, const unsigned short *w, const float *bias,
                   unsigned short *y1, unsigned short *y2, hipStream_t s, int ncu);
// bf16 z-marching weight gradient of the plain 3x3x3 stride-1 conv and its stride-2 twin (conv_bf16w.hip): wgrad16z_plan /
// wgrad16zs_plan above
bool wgrad16z_prologue_ok(const WgradGeom &g);
void wgrad16z_enable(int on);
int pack_weights_batch(int n, const float *const *w, float *const *wf, float *const *wb, float *const *uf, float *const *ub,
                       const int *K, const int *C, const int *T, const int *transposed, hipStream_t s,
                       float *const *vf = nullptr, float *const *vb = nullptr);
int wino_mode();                          // MVD_WINO: 0 off, 1 F(2,3) along W, 2 F(2x2,3x3) (default)
// F(2x2x2,3x3x3) weight gradient (conv_wgrad_wino3.hip): plain 3x3x3 stride-1 conv, 32-multiple channels (wgrad_wino3_plan
// above).  wgrad_wino3_selected: the engine is on and the layer has the minimum of work items per sample;
// wgrad_wino3_ws: partials + bias rows for nsplit splits
bool wgrad_wino3_selected(const WgradGeom &g);
size_t wgrad_wino3_ws(int nsplit, int C, int K);
int wgrad_wino3_enabled();  // MVD_WGRAD_WINO3: 0 off, 1 (default) on
void set_wgrad_wino3_min_items(long n);
void set_wgrad_bias_fold(int on);  // bias gradient inside the narrow-input / transposed-conv weight gradients (< 0: environment)
long wgrad_wino3_launches();  // launches of k_wgrad_wino3 since the library was loaded
// dbias[k] = fp64 sum of the rows pbias[0..nrows)[k] in a fixed order (k_dbias_reduce, conv_mfma.hip)
int dbias_reduce(const float *pbias, float *dbias, int K, int nrows, hipStream_t s);
size_t wino_weight_elems(int C, int K);   // floats of one uf / ub buffer in the active mode

// ConvTranspose3d (kernel == stride) as LDS-free GEMMs (conv_transp.hip); -1 = shape not covered
int convT_fwd_direct(const float *x, const float *wf, const float *bias, float *y, int N, int D, int H, int W, int C, int K,
                     const int st[3], hipStream_t s);
int convT_dgrad_direct(const float *dy, const float *wb, float *dx, int N, int D, int H, int W, int C, int K,
                       const int st[3], hipStream_t s);

int convT_fwd_direct16(const unsigned short *x, const unsigned short *wf, const float *bias, unsigned short *y, int N, int D,
                       int H, int W, int C, int K, const int st[3], hipStream_t s);
int convT_dgrad_direct16(const unsigned short *dy, const unsigned short *wb, unsigned short *dx, int N, int D, int H, int W,
                         int C, int K, const int st[3], hipStream_t s);

// bf16 forward-type engine (conv_bf16.hip): bf16 activations / packed weights, fp32 accumulate, bf16 output
// Optional InstanceNorm fusion of the z-marching kernel k_fwd16z (get_network_from_plans.py:41-44: conv -> InstanceNorm3d
// -> LeakyReLU): `tile_stats` != null asks for the per-workgroup (sum, sum of squares) of the bf16-rounded OUTPUT per
// channel ([N][ntiles][K][2] floats; *ntiles is set to the tiles per sample, or to 0 when the kernel that ran cannot emit
// them); `in_scale` / `in_shift` != null ([N][C1] floats) make the kernel normalise + activate its INPUT while staging it:
// a = bf16(lrelu(fma(x, scale, shift))) -- the InstanceNorm-apply of the producing block folded into this consumer's
// loader (zero padding applies to a, i.e. halo voxels outside the volume stay 0).  `required` = fail (-1) instead of
// running un-fused when the shape does not take the z-marching kernel.
struct Fwd16Fuse {
    float *tile_stats = nullptr;
    int *ntiles = nullptr;
    const float *in_scale = nullptr, *in_shift = nullptr;
    float slope = 0.01f;
};
int fwd_bf16(const FwdGeom &g, const unsigned short *a1, const unsigned short *a2, const unsigned short *w,
             const float *bias, unsigned short *y1, unsigned short *y2, void *ws, size_t ws_bytes, hipStream_t s,
             const Fwd16Fuse *fuse = nullptr);
int fwd16y_enabled();
void fwd16y_enable(int on);
// k_fwd16y (conv_bf16y.hip): -1 = not this kernel's shape; stats_tiles_only != null = query (no launch)
int launch_fwd16y(const FwdGeom &g, const unsigned short *a1, const unsigned short *a2, const unsigned short *w,
                  const float *bias, unsigned short *y1, unsigned short *y2, hipStream_t s, const Fwd16Fuse *fuse, int ncu,
                  int *stats_tiles_only);
// tiles per sample the z-marching kernel would emit statistics for (0: this shape does not run on it)
int fwd_bf16_stats_tiles(const FwdGeom &g);
// 1 when the shape runs on a kernel that has the InstanceNorm input prologue (Fwd16Fuse::in_scale / in_shift)
int fwd_bf16_prologue_ok(const FwdGeom &g);
int pack_weight16(const float *w, unsigned short *wf, unsigned short *wb, int K, int C, int T, int transposed,
                  hipStream_t s);
int pack_weights16_batch(int n, const float *const *w, unsigned short *const *wf, unsigned short *const *wb, const int *K,
                         const int *C, const int *T, const int *transposed, const int *Csrc, hipStream_t s);

}  // namespace mvd
