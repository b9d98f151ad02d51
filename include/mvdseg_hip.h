/* mvdseg_hip.h -- C ABI of libmvdseg_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the one
 * data-parallel hot path of JaronTu/Multimodal_MVD_Seg: the nnU-Net-v2 3d_fullres PlainConvUNet train step
 * (SURVEY.md section 8).  The reference has NO FFI on this path (it calls torch.nn -> ATen -> cuDNN/MIOpen);
 * every entry point below cites the reference call site whose arithmetic it replaces.
 *
 * Conventions
 *  - plain pointers and sizes only; all pointers are DEVICE pointers owned by the caller (the PyTorch caching
 *    allocator on the Python side).  The library never allocates or frees device memory and keeps no pointer
 *    across calls.  `stream` is a hipStream_t passed as void* (the caller's current stream).
 *  - return 0 on success, non-zero otherwise; no exception crosses the ABI; mvd_last_error() returns the
 *    thread-local message of the last failing call.
 *  - activations are NDHWC fp32 ("channels last 3d"): x[n][d][h][w][c].  Logits, targets and the 1-channel maps
 *    of the topology losses are planar NCDHW fp32.  Weights cross the boundary in torch layout
 *    (Conv3d [K][C][kd][kh][kw], ConvTranspose3d [C][K][kd][kh][kw]); mvd_pack_* builds the tap-major shadow
 *    copies the kernels stream.
 *  - every reduction is a fixed-order two-stage reduce (no float atomics): results are run-to-run bit-identical.
 *  - workspaces: caller passes `ws` / `ws_bytes`; mvd_*_workspace_bytes() returns the requirement.
 */
#ifndef MVDSEG_HIP_H
#define MVDSEG_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVD_VERSION 100 /* 0.1.0 */
#define MVD_MAX_TAPS 27

int mvd_version(void);
const char *mvd_last_error(void);
/* 1 if the build contains the MFMA implicit-GEMM engine (it always does; kept for host-side asserts) */
int mvd_has_mfma(void);
/* force the scalar gather kernels (debug / cross-check): 0 = auto (MFMA when shapes allow), 1 = scalar only */
int mvd_set_conv_engine(int mode);
/* debug/test hook: minimum number of 128-voxel x 32-channel work items for the Winograd conv kernel (n < 0: default) */
int mvd_set_wino_min_items(long n);

/* ------------------------------------------------------------------------------------------------------------
 * Weight packing.  torch Conv3d weight [K][C][T] (T = kd*kh*kw taps, row-major) ->
 *   wf[T][C][K]  (forward: reduce over C, produce K)      wb[T][K][C]  (dgrad: reduce over K, produce C)
 * `transposed` != 0: source is a ConvTranspose3d weight [C][K][T] (same two outputs).
 * Replaces nothing in the reference (torch keeps one layout); it is the price of the tap-major layout. */
int mvd_pack_weight(const float *w, float *wf, float *wb, int K, int C, int T, int transposed, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Conv3d, kernel k[a] in {1,3}, padding (k-1)/2, stride s[a] in {1,2}, dilation 1 (K1/K5/K6 of SURVEY 2.4).
 * Replaces torch.nn.Conv3d inside every ConvDropoutNormReLU (get_network_from_plans.py:39-45,
 * UNetDecoder.py:61-65) and the decoder's torch.cat((x, skip), 1) (UNetDecoder.py:107): the input is the channel
 * concatenation of x1 [N,D,H,W,C1] and x2 [N,D,H,W,C2] (x2 may be NULL with C2 = 0).
 *   y[n,o,k] = bias[k] + sum_t sum_c x[n, o*s + t - pad, c] * wf[t][c][k],   y: [N,Do,Ho,Wo,K]
 * Do = (D + 2*pad - k)/s + 1. */
/* ws (optional, may be NULL): scratch for the split-reduce path the engine takes on skinny problems (few output
 * voxels, hundreds of reduce channels: the 8^3 / 4^3 stages); size from mvd_conv_fwd_workspace_bytes(N, output voxels
 * per sample, output channels).  Same for dgrad / convT fwd / convT dgrad (output = the tensor being produced). */
size_t mvd_conv_fwd_workspace_bytes(int N, long out_voxels, int K);
int mvd_conv3d_fwd(const float *x1, int C1, const float *x2, int C2, const float *wf, const float *bias, float *y,
                   int N, int D, int H, int W, int K, const int ksize[3], const int stride[3], void *ws,
                   size_t ws_bytes, void *stream);
/* dgrad: dx = conv_transpose(dy, w); written as dx1 [.,C1] and dx2 [.,C2] (channel split of the concat). */
int mvd_conv3d_dgrad(const float *dy, const float *wb, float *dx1, int C1, float *dx2, int C2, int N, int D, int H,
                     int W, int K, const int ksize[3], const int stride[3], void *ws, size_t ws_bytes, void *stream);
/* wgrad: dw in TORCH layout [K][C1+C2][T], dbias [K] (may be NULL).  Fixed-order split reduction through `ws`. */
/* Winograd engines of the two entries above for 3x3x3 stride-1 convs with C % 32 == 0, K % 32 == 0 (every conv of
 * the network but the input layer and the strided ones): F(2x2,3x3) over H and W -- 4/9 of the multiply-adds of
 * the direct form (env MVD_WINO=1 selects F(2,3) along W only: 2/3) -- fp32 throughout, same results within fp32
 * round-off (tests: <= 1e-5 relative to fp64).
 * mvd_pack_weight_wino: torch weight [K][C][3][3][3] -> uf (forward) / ub (input gradient), mvd_wino_weight_elems(C, K)
 * floats each, in the MFMA operand order of the active mode.
 *
 * One route for every fp32 conv.  An engine takes a pass (the forward, or the input gradient) when its predicate holds:
 * kernel size, stride 1, 32-multiple channels and its minimum of work items; the mvd_conv_*_applicable queries return the
 * predicate of one engine as forward (1) | input gradient (2) bits, and mvd_conv3d_route names the preferred engine of both
 * passes (forward kind in bits 0-3, input-gradient kind in bits 4-7): F(2x2x2,3x3x3) over F(2x2,3x3), the in-plane engine
 * for 1x3x3, direct otherwise.  mvd_conv3d_fwd_routed / mvd_conv3d_dgrad_routed are mvd_conv3d_fwd / mvd_conv3d_dgrad with a
 * Winograd table and its kind: the table's engine runs if and only if its predicate holds for the pass, the direct engines
 * (same results) otherwise -- strides, 1x1x1, too few work items, table == NULL.  An in-plane table requires kernel size
 * (1,3,3).
 * Statistics epilogue of the forward ("optional sum x / sum x^2 epilogue"): stats == NULL: none.  stats_tiles == 0:
 * that of the F(2x2,3x3) / F(2x2x2,3x3x3) kernels, per-tile (sum y, sum y^2) per output channel to stats
 * [N][mvd_conv_stats_tiles(D,H,W)][K][2] floats.  stats_tiles > 0: that of the direct engines, stats [N][stats_tiles][K][2]
 * with stats_tiles from mvd_conv3d_fwd_stats_tiles (below; the table is not used).  stats_done is required with stats:
 * *stats_done = 1 when they were written (0: not produced, run the plain norm). */
#define MVD_CONV_DIRECT 0
#define MVD_CONV_WINO2 1  /* F(2x2,3x3), table of mvd_pack_weight_wino */
#define MVD_CONV_WINO3 2  /* F(2x2x2,3x3x3), table of mvd_pack_weight_wino3 */
#define MVD_CONV_WINO2P 3 /* F(2x2,3x3) of a 1x3x3 kernel, table of mvd_pack_weight_wino2p */
int mvd_conv3d_route(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3], const int stride[3]);
int mvd_conv3d_fwd_routed(const float *x1, int C1, const float *x2, int C2, const float *wf, const float *table, int table_kind,
                          const float *bias, float *y, float *stats, long stats_tiles, int *stats_done, int N, int D, int H,
                          int W, int K, const int ksize[3], const int stride[3], void *ws, size_t ws_bytes, void *stream);
int mvd_conv3d_dgrad_routed(const float *dy, const float *wb, const float *table, int table_kind, float *dx1, int C1, float *dx2,
                            int C2, int N, int D, int H, int W, int K, const int ksize[3], const int stride[3], void *ws,
                            size_t ws_bytes, void *stream);
/* bit 0: the forward would use the Winograd kernel, bit 1: the input gradient would (0: skip packing uf/ub) */
int mvd_conv_wino_applicable(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3], const int stride[3]);
/* floats in one uf / ub buffer (48*C*K for the default F(2x2,3x3) mode, 36*C*K for F(2,3) along W) */
size_t mvd_wino_weight_elems(int C, int K);
/* 0 = direct engines only, 1 = F(2,3) along W, 2 = F(2x2,3x3) over H and W (default; env MVD_WINO) */
int mvd_wino_mode(void);
int mvd_pack_weight_wino(const float *w, float *uf, float *ub, int K, int C, void *stream);
/* mvd_conv3d_fwd_routed with uf as an F(2x2,3x3) table (uf == NULL: the direct engines) and no statistics */
int mvd_conv3d_fwd_wino(const float *x1, int C1, const float *x2, int C2, const float *wf, const float *uf,
                        const float *bias, float *y, int N, int D, int H, int W, int K, const int ksize[3],
                        const int stride[3], void *ws, size_t ws_bytes, void *stream);
/* tiles per sample of the Winograd engines' statistics epilogue (4x4x8 voxels each) */
size_t mvd_conv_stats_tiles(int D, int H, int W);
/* F(2x2x2,3x3x3) engine: Winograd F(2,3) along D as well -- 8 multiply-adds per output and channel pair instead of the
 * 12 of F(2x2,3x3) -- same coefficients (1 and 1/2), same results within fp32 round-off.  It refines the F(2x2,3x3)
 * engine: mvd_conv_wino3_applicable returns the bits of mvd_conv_wino_applicable for which the 3-D kernel also has
 * its own minimum of work items PER SAMPLE (4x8x8 voxels x 32 output channels, default 128: the choice does not
 * depend on the batch size; mvd_set_wino3_min_items, < 0 restores the default) and is on (env MVD_WINO3=0 turns it off; the F(2x2,3x3) entries above keep their meaning in every case).
 * mvd_pack_weight_wino3: torch weight -> vf (forward) / vb (input gradient), mvd_wino3_weight_elems(C, K) = 64*C*K
 * floats each; the statistics epilogue writes the layout of the F(2x2,3x3) kernel.
 * mvd_pack_weights_batch3: every conv weight of a network re-packed in ONE launch (the per-layer pack entries are
 * launch-bound; called by the fused optimizer right after the update).  Host tables of n jobs: w[q] the torch-layout
 * weight, wf / wb the mvd_pack_weight outputs, uf / ub the mvd_pack_weight_wino outputs (need MVD_WINO=2), vf / vb the 3-D
 * tables; null entries are skipped. */
int mvd_set_wino3_min_items(long n);
int mvd_conv_wino3_applicable(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3], const int stride[3]);
size_t mvd_wino3_weight_elems(int C, int K);
int mvd_pack_weight_wino3(const float *w, float *vf, float *vb, int K, int C, void *stream);
int mvd_pack_weights_batch3(int n, const float *const *w, float *const *wf, float *const *wb, float *const *uf,
                            float *const *ub, float *const *vf, float *const *vb, const int *K, const int *C,
                            const int *T, const int *transposed, void *stream);
/* The same epilogue in the direct fp32 engines (the narrow-input / chunked kernel k_fwd_mfma and the stride-2 kernel
 * k_fwd32s; a tile is one wave's plane of the workgroup tile, at most 64 values).  mvd_conv3d_fwd_stats_tiles: tiles per
 * sample of the kernel that would run for this conv, 0 when it has no epilogue: the stats_tiles of mvd_conv3d_fwd_routed (a
 * conv that would split its reduce channels over workgroups runs unsplit then: ask only where a statistics pass would run
 * otherwise). */
long mvd_conv3d_fwd_stats_tiles(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3], const int stride[3]);
/* F(2x2,3x3) engine of the 9-tap in-plane layers: kernel size (1,3,3), stride 1, 32-multiple channels -- the convs of a 2-D
 * network seen as [N,C,1,H,W] and the in-plane layers of anisotropic 3-D plans (4 multiply-adds per output and channel
 * pair instead of 9).  Other 9-tap kernels, e.g. (3,3,1), keep the direct engine.  mvd_conv_wino2p_applicable: forward (1)
 * | input gradient (2) bits for which the kernel has its minimum of work items (4 planes x 4 x 8 outputs x 32 produced
 * channels over all N*D planes; mvd_set_wino2p_min_items, < 0 restores the default, a huge value turns the kernel off; env
 * MVD_WINO2P_MIN, MVD_WINO=0).  mvd_pack_weight_wino2p: torch weight [K][C][1][3][3] -> pf (forward) / pb (input gradient),
 * mvd_wino2p_weight_elems(C, K) = 16*C*K floats each; in mvd_pack_weights_batch3 a job with T = 9 takes them as uf / ub.
 * No statistics epilogue.  mvd_conv_wino2p_applicable judges the shape alone: a call whose pointers are not
 * 16-byte aligned, or with more than 2^30 work items or K*32 >= 2^27, also falls back to the direct engines (same
 * results) although the bits were set. */
int mvd_set_wino2p_min_items(long n);
int mvd_conv_wino2p_applicable(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3], const int stride[3]);
size_t mvd_wino2p_weight_elems(int C, int K);
int mvd_pack_weight_wino2p(const float *w, float *pf, float *pb, int K, int C, void *stream);
/* F(2x2x2,3x3x3) weight gradient: mvd_conv3d_wgrad runs it for fp32 3x3x3 stride-1 convs with 32-multiple channels
 * (two inputs included) that have at least the minimum of work items PER SAMPLE (2x8x8 dy voxels x 32 input x 32
 * output channels; mvd_set_wgrad_wino3_min_items, < 0 restores the default) unless MVD_WGRAD_WINO3=0 or MVD_WINO=0.
 * mvd_conv_wgrad_wino3_applicable: 1 when it would run for that shape, else 0.  mvd_wgrad_wino3_launches: its launches
 * since the library was loaded (a workspace too small for it falls back to F(2x2,3x3) without an error). */
int mvd_set_wgrad_wino3_min_items(long n);
int mvd_conv_wgrad_wino3_applicable(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3],
                                    const int stride[3]);
long mvd_wgrad_wino3_launches(void);
/* The fp32 weight gradients of the narrow-input layer (k_wgrad_smallc: an idle GEMM row with a ones operand) and of the
 * transposed convs (k_wgrad_mfma: plain adds on the dy fragments each wave stages) also produce the bias gradient, so no
 * column-sum pass over dy runs for them (the workspace must hold the extra rows, mvd_conv*_wgrad_workspace_bytes; the
 * column-sum pass runs otherwise).  MVD_WGRAD_BIAS_FOLD=0 / mvd_set_wgrad_bias_fold(0) restore the separate pass (< 0:
 * back to the environment); dw does not depend on it. */
int mvd_set_wgrad_bias_fold(int on);
/* What a weight-gradient entry point runs for a shape: the host-only plan the launch code itself consumes (no device call).
 * transposed 0: mvd_conv3d_wgrad[_bf16] (prologue 1: mvd_conv3d_wgrad_bf16_fused); 1: mvd_convT3d_wgrad[_bf16] of an
 * [N,D,H,W,C1] input (ksize ignored, C2 = 0).  ws_bytes 0 = what the matching workspace query returns.  want_bias: dbias is
 * asked for.  Returns 0, or 2 with mvd_last_error for arguments the entry points refuse.  plan[MVD_WG_PLAN_LEN]:
 *   0 kernel (MVD_WG_*), 1 reduce kernel (MVD_WGR_*), 2 source of the bias gradient (MVD_WGB_*),
 *   3..7 template configuration TPW, NA, NB, SH, TRI (k_wgrad_wino<NA, NB, NQ>: NQ as TPW; 0 where a kernel has none),
 *   8..10 tile TD, TH, TW and 11..13 tiles ntd, nth, ntw per sample, 14 ntiles (the z-marching kernels: planes per chunk
 *   zc x 8 (stride 2: 4) x 32 columns, chunks nzc and column tiles per sample, 14 their units; the scalar kernel: 14 voxels),
 *   15 nsplit (split-K workgroups), 16 partial tensors each of them writes, 17 ncb, 18 nkb (channel blocks of the grid),
 *   19 bias rows [K] behind the partials (0: none), 20 workspace bytes the path touches, 21 workspace bytes planned for,
 *   22.. the switches it read: 22 MVD_WINO mode, 23 wino3 enabled, 24 wino3 minimum items, 25 bias fold, 26 bf16 kernel
 *   (mvd_set_bf16_wgrad_kernel), 27 scalar engine mode, 28 MVD_WGRAD16_BIG, 29 MVD_WGRAD16_TRI, 30 MVD_WGRAD_DB,
 *   31 MVD_WGRAD16Z, 32 MVD_WGRAD16ZS, 33 MVD_WGRAD_REDUCE_G16.
 * fp32 operands that are not 16-byte aligned take MVD_WG_SCALAR whatever the plan says (bf16: refused).
 * mvd_conv_wgrad_last_kernel: the MVD_WG_* id stored at the launch site by the latest weight-gradient call of the process. */
#define MVD_WG_NONE 0
#define MVD_WG_WINO3 1     /* k_wgrad_wino3: fp32 F(2x2x2,3x3x3) */
#define MVD_WG_WINO2W12 2  /* k_wgrad_wino2w12: fp32 F(2x2,3x3) */
#define MVD_WG_WINO 3      /* k_wgrad_wino: fp32 F(2,3) along W (MVD_WINO=1) */
#define MVD_WG_SMALLC 4    /* k_wgrad_smallc: fp32 narrow input */
#define MVD_WG_MFMA 5      /* k_wgrad_mfma: fp32 generic */
#define MVD_WG_WGRAD16 6   /* k_wgrad16: bf16 tiled */
#define MVD_WG_WGRAD16Z 7  /* k_wgrad16z: bf16 z-marching, stride 1 */
#define MVD_WG_WGRAD16ZS 8 /* k_wgrad16zs: bf16 z-marching, stride 2 */
#define MVD_WG_SCALAR 9    /* k_wgrad_scalar */
#define MVD_WG_PLAN_LEN 34
#define MVD_WGR_F4 1    /* k_wgrad_reduce_f<4> */
#define MVD_WGR_F16 2   /* k_wgrad_reduce_f<16> */
#define MVD_WGR_WINO 3  /* k_wgrad_reduce_wino */
#define MVD_WGR_WINO2 4 /* k_wgrad_reduce_wino2 */
#define MVD_WGR_WINO3 5 /* k_wgrad_reduce_wino3 */
#define MVD_WGR_D 6     /* k_wgrad_reduce_d (fp64 partials of the scalar kernel) */
#define MVD_WGB_NONE 0     /* no dbias asked for */
#define MVD_WGB_COLSUM 1   /* the column-sum pass over dy */
#define MVD_WGB_GENERIC 2  /* k_wgrad_mfma, every tap on one dy slot: 4 rows per split */
#define MVD_WGB_CONVT 3    /* k_wgrad_mfma, transposed conv: 16 rows per split */
#define MVD_WGB_SMALLC 4   /* k_wgrad_smallc: the idle GEMM row */
#define MVD_WGB_WINO3 5    /* k_wgrad_wino3: 2 rows per split */
#define MVD_WGB_WINO2W12 6 /* k_wgrad_wino2w12: 2 rows per split */
#define MVD_WGB_SLOT28 7   /* k_wgrad16: the idle 28th tap slot */
#define MVD_WGB_ZMARCH 8   /* k_wgrad16z: one row per split */
int mvd_conv_wgrad_plan(int transposed, int is_bf16, int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3],
                        const int stride[3], size_t ws_bytes, int want_bias, int prologue, long *plan);
int mvd_conv_wgrad_last_kernel(void);
size_t mvd_conv3d_wgrad_workspace_bytes(int C, int K, int T, int N, int Do, int Ho, int Wo);
int mvd_conv3d_wgrad(const float *x1, int C1, const float *x2, int C2, const float *dy, float *dw, float *dbias,
                     int N, int D, int H, int W, int K, const int ksize[3], const int stride[3], void *ws,
                     size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * ConvTranspose3d with kernel == stride (non-overlapping; K2).  Replaces the decoder's transpconvs
 * (UNetDecoder.py:56-59,106).  x: [N,D,H,W,C] -> y: [N,D*s0,H*s1,W*s2,K];  wf[T][C][K], T = s0*s1*s2.
 *   y[n, q*s + p, k] = bias[k] + sum_c x[n,q,c] * w[c][k][p] */
int mvd_convT3d_fwd(const float *x, const float *wf, const float *bias, float *y, int N, int D, int H, int W, int C,
                    int K, const int stride[3], void *ws, size_t ws_bytes, void *stream);
int mvd_convT3d_dgrad(const float *dy, const float *wb, float *dx, int N, int D, int H, int W, int C, int K,
                      const int stride[3], void *ws, size_t ws_bytes, void *stream);
size_t mvd_convT3d_wgrad_workspace_bytes(int C, int K, int T, int N, int D, int H, int W);
/* dw in TORCH layout [C][K][T], dbias [K] */
int mvd_convT3d_wgrad(const float *x, const float *dy, float *dw, float *dbias, int N, int D, int H, int W, int C,
                      int K, const int stride[3], void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * bf16 mixed precision (BASELINE cfg 4/5: the reference's autocast path, nnUNetTrainer.py:906): activations and
 * packed weights are bf16 (uint16_t storage), accumulation and bias fp32, outputs bf16; master weights and all
 * weight gradients stay fp32.  C % 32 == 0 and K % 32 == 0 (the 4-modality input layer: mvd_pad_channels_bf16 first).
 * mvd_pack_weight_bf16: torch fp32 weight -> wf16 (reduce C, produce K) / wb16 (reduce K, produce C), layout
 * [chunk32][tap][kstep][lane half][out channel][8]. */
int mvd_pack_weight_bf16(const float *w, uint16_t *wf, uint16_t *wb, int K, int C, int T, int transposed, void *stream);
/* Every bf16 pack of a network in ONE launch (called by the fused optimizer after its update, like
 * mvd_pack_weights_batch3 for the fp32 layouts): host tables of n jobs, outputs bit-identical to mvd_pack_weight_bf16. */
int mvd_pack_weights_bf16_batch(int n, const float *const *w, uint16_t *const *wf, uint16_t *const *wb, const int *K,
                                const int *C, const int *T, const int *transposed, void *stream);
/* The same launch with a source channel count per job: job q reads a [K][Csrc][T] weight and packs it as the [K][C][T]
 * weight whose reduce channels Csrc .. C-1 are zero (the 4-modality input conv, run on the 32-channel engines) --
 * bit-identical to mvd_pack_weight_bf16 of the zero-padded tensor.  Csrc == C: the plain job; Csrc < C: conv weights only. */
int mvd_pack_weights_bf16_batch_pad(int n, const float *const *w, uint16_t *const *wf, uint16_t *const *wb, const int *K,
                                    const int *C, const int *T, const int *transposed, const int *Csrc, void *stream);
int mvd_conv3d_fwd_bf16(const uint16_t *x1, int C1, const uint16_t *x2, int C2, const uint16_t *wf, const float *bias,
                        uint16_t *y, int N, int D, int H, int W, int K, const int ksize[3], const int stride[3],
                        void *ws, size_t ws_bytes, void *stream);
int mvd_conv3d_dgrad_bf16(const uint16_t *dy, const uint16_t *wb, uint16_t *dx1, int C1, uint16_t *dx2, int C2, int N,
                          int D, int H, int W, int K, const int ksize[3], const int stride[3], void *ws, size_t ws_bytes,
                          void *stream);
int mvd_convT3d_fwd_bf16(const uint16_t *x, const uint16_t *wf, const float *bias, uint16_t *y, int N, int D, int H, int W,
                         int C, int K, const int stride[3], void *ws, size_t ws_bytes, void *stream);
int mvd_convT3d_dgrad_bf16(const uint16_t *dy, const uint16_t *wb, uint16_t *dx, int N, int D, int H, int W, int C, int K,
                           const int stride[3], void *ws, size_t ws_bytes, void *stream);
/* weight gradients from bf16 activations / bf16 dy: operands widened to fp32 in registers, fp32 MFMA, fp32 partials,
 * fp64 fixed-order reduce -> fp32 dw (torch layout) and fp32 dbias.  Workspace sizes: the fp32 queries above. */
int mvd_conv3d_wgrad_bf16(const uint16_t *x1, int C1, const uint16_t *x2, int C2, const uint16_t *dy, float *dw,
                          float *dbias, int N, int D, int H, int W, int K, const int ksize[3], const int stride[3],
                          void *ws, size_t ws_bytes, void *stream);
int mvd_convT3d_wgrad_bf16(const uint16_t *x, const uint16_t *dy, float *dw, float *dbias, int N, int D, int H, int W,
                           int C, int K, const int stride[3], void *ws, size_t ws_bytes, void *stream);
/* The fused block of the north_star in bf16 -- Conv3d 3x3x3 -> InstanceNorm3d(affine) -> LeakyReLU
 * (get_network_from_plans.py:41-44; block composition UNetDecoder.py:61-65 / PlainConvEncoder) -- on the z-marching
 * conv kernel (3x3x3, stride 1, 32 -> 32 channels, large volumes):
 *   mvd_conv3d_fwd_bf16_stats_tiles: tiles per sample the conv would emit statistics for (0: this shape runs on a kernel
 *     without the epilogue; the caller then uses mvd_instnorm_lrelu_fwd_bf16).
 *   mvd_conv3d_fwd_bf16_fused: mvd_conv3d_fwd_bf16 plus
 *     - tile_stats != NULL: per-workgroup (sum, sum of squares) of the bf16-rounded output per channel,
 *       [N][*ntiles_out][K][2] floats (*ntiles_out = 0 on return: the kernel that ran has no epilogue);
 *     - in_scale / in_shift != NULL ([N][C1] floats): the INPUT is the raw output of the producing conv and is
 *       normalised + activated while it is staged, a = bf16(lrelu(fma(x, scale, shift))) with zero padding applied to a
 *       -- the producing block's InstanceNorm-apply + LeakyReLU folded into this consumer's loader, so the activated
 *       tensor is never written to HBM.  Error 3 when the shape does not take the z-marching kernel.
 *   mvd_instnorm_finalize_tiles: tile statistics -> mean, rstd (biased variance, eps inside the root), scale = gamma*rstd,
 *     shift = beta - mean*scale; one launch, fp64, fixed order.
 *   mvd_instnorm_lrelu_apply_bf16: y = bf16(lrelu(fma(x, scale, shift))) -- the same arithmetic as the fused prologue, for
 *     the consumers that have none.  The backward pass is mvd_instnorm_lrelu_bwd_bf16 on (x, mean, rstd). */
int mvd_conv3d_fwd_bf16_stats_tiles(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3],
                                    const int stride[3]);
/* Gradient of a tensor with TWO consumers (a skip connection: the next encoder stage's strided conv and the decoder conv
 * that reads it as its second pointer, UNetDecoder.py:106-108): the consumer whose backward runs second adds its input
 * gradient into the buffer the first one wrote, inside its own kernel, instead of autograd's separate elementwise add.
 *   mvd_conv3d_dgrad_acc_ok: 1 when an accumulating kernel exists for the conv (3x3x3, stride 2, 32-multiple channels).
 *   mvd_conv3d_dgrad_acc / _bf16_acc: dx1 += input gradient (fp32: a + b as torch's add; bf16: fp32 add of the two bf16
 *   values, one rounding, as torch's bf16 add). */
int mvd_conv3d_dgrad_acc_ok(int is_bf16, int N, int D, int H, int W, int C1, int K, const int ksize[3], const int stride[3]);
int mvd_conv3d_dgrad_acc(const float *dy, const float *wb, float *dx1, int C1, int N, int D, int H, int W, int K,
                         const int ksize[3], const int stride[3], void *stream);
int mvd_conv3d_dgrad_bf16_acc(const uint16_t *dy, const uint16_t *wb, uint16_t *dx1, int C1, int N, int D, int H, int W, int K,
                              const int ksize[3], const int stride[3], void *ws, size_t ws_bytes, void *stream);
/* which z-marching kernel serves the 3x3x3 stride-1 convs with 32 produce channels at the patch resolution: 1 (default,
 * MVD_FWD16Y) = k_fwd16y (16x16x32 tiles; 32 or 64 reduce channels; statistics epilogue and loader prologue), 0 =
 * k_fwd16z (32x32x16 tiles, 32 reduce channels, loader prologue only).  A/B and cross-check switch. */
int mvd_set_bf16_zmarch_kernel(int which);
/* which kernel computes the bf16 weight gradient of the plain 3x3x3 stride-1 convs on volumes at least 32 wide
 * (nnUNetTrainer.py:888-925 backward): 1 (default, MVD_WGRAD16Z) = k_wgrad16z (z-marching column, csrc/conv_bf16w.hip),
 * 0 = k_wgrad16 (4x8x8 tiles).  A/B and cross-check switch. */
int mvd_set_bf16_wgrad_kernel(int which);
/* Weight gradient with the loader prologue (ops.NormActConv3dFn.backward; get_network_from_plans.py:41-44 fused block, the
 * backward of nnUNetTrainer.py:888-925): x1 is the RAW bf16 output of the producing conv, the operand of the product is
 * lrelu(x1 * in_scale[n][c] + in_shift[n][c]) rounded to bf16 -- bit-identical to mvd_conv3d_wgrad_bf16 over the tensor
 * mvd_instnorm_lrelu_apply_bf16 would write, which therefore need not exist.  _prologue_ok: 1 when the shape is served. */
int mvd_conv3d_wgrad_bf16_prologue_ok(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3], const int stride[3]);
int mvd_conv3d_wgrad_bf16_fused(const uint16_t *x1, int C1, const uint16_t *dy, float *dw, float *dbias, int N, int D, int H, int W,
                                int K, const int ksize[3], const int stride[3], const float *in_scale, const float *in_shift,
                                float slope, void *ws, size_t ws_bytes, void *stream);
/* 1 when mvd_conv3d_fwd_bf16_fused accepts in_scale / in_shift for this shape (a kernel with the loader prologue runs it) */
int mvd_conv3d_fwd_bf16_prologue_ok(int N, int D, int H, int W, int C1, int C2, int K, const int ksize[3],
                                    const int stride[3]);
int mvd_conv3d_fwd_bf16_fused(const uint16_t *x1, int C1, const uint16_t *x2, int C2, const uint16_t *wf, const float *bias,
                              uint16_t *y, int N, int D, int H, int W, int K, const int ksize[3], const int stride[3],
                              const float *in_scale, const float *in_shift, float slope, float *tile_stats, int *ntiles_out,
                              void *ws, size_t ws_bytes, void *stream);
int mvd_instnorm_finalize_tiles(const float *tile_stats, long ntiles, const float *gamma, const float *beta, float *mean,
                                float *rstd, float *scale, float *shift, int N, long V, int C, float eps, void *stream);
int mvd_instnorm_lrelu_apply_bf16(const uint16_t *x, const float *scale, const float *shift, uint16_t *y, int N, long V,
                                  int C, float slope, void *stream);
/* statistics pass alone (for a conv whose kernel has no epilogue): mean, rstd and scale / shift of x (fp32 or bf16 NDHWC);
 * workspace: mvd_instnorm_workspace_bytes */
int mvd_instnorm_stats_bf16(const void *x, int x_is_bf16, const float *gamma, const float *beta, float *mean, float *rstd,
                            float *scale, float *shift, int N, long V, int C, float eps, void *ws, size_t ws_bytes,
                            void *stream);
/* InstanceNorm+LeakyReLU with bf16 output (statistics and arithmetic fp32/fp64 as in the fp32 entry points).
 * x is fp32 (x_is_bf16 == 0: the first, fp32, conv of the network) or bf16; y and dy are bf16; dx has x's type.
 * Workspace: mvd_instnorm_workspace_bytes.  C % 4 == 0. */
int mvd_instnorm_lrelu_fwd_bf16(const void *x, int x_is_bf16, const float *gamma, const float *beta, uint16_t *y,
                                float *mean, float *rstd, int N, long V, int C, float eps, float slope, void *ws,
                                size_t ws_bytes, void *stream);
int mvd_instnorm_lrelu_bwd_bf16(const void *x, int x_is_bf16, const uint16_t *dy, const float *gamma, const float *beta,
                                const float *mean, const float *rstd, void *dx, float *dgamma, float *dbeta, int N,
                                long V, int C, float slope, void *ws, size_t ws_bytes, void *stream);
/* seg head on bf16 activations: fp32 weights, fp32 planar logits (the loss kernels stay fp32), bf16 dx, fp32 dw/dbias */
int mvd_seghead_fwd_bf16(const uint16_t *x, const float *w, const float *bias, float *logits, int N, long V, int C,
                         int K, void *stream);
int mvd_seghead_bwd_bf16(const uint16_t *x, const float *w, const float *dlogits, uint16_t *dx, float *dw, float *dbias,
                         int N, long V, int C, int K, int accumulate, void *ws, size_t ws_bytes, void *stream);
/* The seg head of the LAST decoder stage reading the RAW bf16 output of that stage's last conv (UNetDecoder.py:110 after
 * get_network_from_plans.py:41-44): a = bf16(lrelu(x * scale[n][c] + shift[n][c])) is applied in the loaders, the activated
 * tensor is not materialised.  _bwd: dx = d a (the caller runs the InstanceNorm backward on it), dw / dbias over the
 * re-computed a.  Bit-identical to mvd_seghead_*_bf16 over the tensor mvd_instnorm_lrelu_apply_bf16 would write: the
 * forward runs the kernel mvd_seghead_fwd_path names for the shape (one thread or 2 / 4 / 8 lanes per voxel), with the
 * loader prologue. */
int mvd_seghead_bf16_fused_ok(int N, long V, int C, int K);
/* fp32 twins (mean / rstd / gamma / beta: the arithmetic of the fp32 apply pass); same eligibility query */
int mvd_seghead_fwd_fused(const float *x, const float *mean, const float *rstd, const float *gamma, const float *beta, float slope,
                          const float *w, const float *bias, float *logits, int N, long V, int C, int K, void *stream);
int mvd_seghead_bwd_fused(const float *x, const float *mean, const float *rstd, const float *gamma, const float *beta, float slope,
                          const float *w, const float *dlogits, float *dx, float *dw, float *dbias, int N, long V, int C, int K,
                          int accumulate, void *ws, size_t ws_bytes, void *stream);
/* mean / rstd from the fp32 conv epilogue's tile statistics without the apply pass (the first half of
 * mvd_instnorm_lrelu_fwd_prestats) */
int mvd_instnorm_stats_from_tiles(const float *tile_stats, long ntiles, float *mean, float *rstd, int N, long V, int C, float eps,
                                  void *ws, size_t ws_bytes, void *stream);
int mvd_seghead_fwd_bf16_fused(const uint16_t *x, const float *scale, const float *shift, float slope, const float *w,
                               const float *bias, float *logits, int N, long V, int C, int K, void *stream);
int mvd_seghead_bwd_bf16_fused(const uint16_t *x, const float *scale, const float *shift, float slope, const float *w,
                               const float *dlogits, uint16_t *dx, float *dw, float *dbias, int N, long V, int C, int K,
                               int accumulate, void *ws, size_t ws_bytes, void *stream);
/* flat conversions (round-to-nearest-even) for tensors that cross the precision boundary (distillation features) */
int mvd_cast_f32_to_bf16(const float *src, uint16_t *dst, long n, void *stream);
int mvd_cast_bf16_to_f32(const uint16_t *src, float *dst, long n, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * InstanceNorm3d(eps, affine) + LeakyReLU(slope), fused (K3/K4).  Replaces nn.InstanceNorm3d + nn.LeakyReLU of
 * every ConvDropoutNormReLU (get_network_from_plans.py:41-44).  x,y: [N,V,C] NDHWC with V = D*H*W.
 * Biased variance over V, no running stats.  mean/rstd [N][C] are outputs (saved for backward).
 * ws: 2*N*nblk*C doubles (nblk from mvd_instnorm_nblk).
 * Alignment (every InstanceNorm entry point, fp32 and bf16): for C % 4 == 0 the kernels load and store four channels at a
 * time, so x, y, dy and dx must be 16-byte aligned as fp32 and 8-byte aligned as bf16; a pointer that is not is refused
 * before any launch.  C % 4 != 0 has no such requirement, nor has the planar logit gradient of mvd_instnorm_lrelu_bwd_head. */
int mvd_instnorm_nblk(int N, long V, int C);
size_t mvd_instnorm_workspace_bytes(int N, long V, int C);
int mvd_instnorm_lrelu_fwd(const float *x, const float *gamma, const float *beta, float *y, float *mean,
                           float *rstd, int N, long V, int C, float eps, float slope, void *ws, size_t ws_bytes,
                           void *stream);
/* dx [N,V,C]; dgamma/dbeta [C] (overwritten).  Recomputes z = xhat*gamma+beta from x for the LeakyReLU mask. */
/* forward with the statistics taken from the producing conv's epilogue (mvd_conv3d_fwd_routed): no pass over x
 * for mean / variance; everything else as mvd_instnorm_lrelu_fwd */
int mvd_instnorm_lrelu_fwd_prestats(const float *x, const float *tile_stats, long ntiles, const float *gamma,
                                    const float *beta, float *y, float *mean, float *rstd, int N, long V, int C, float eps,
                                    float slope, void *ws, size_t ws_bytes, void *stream);
int mvd_instnorm_lrelu_bwd(const float *x, const float *dy, const float *gamma, const float *beta,
                           const float *mean, const float *rstd, float *dx, float *dgamma, float *dbeta, int N,
                           long V, int C, float slope, void *ws, size_t ws_bytes, void *stream);
/* Small volumes run ONE launch per direction (a workgroup keeps 16 channels of a sample in registers: x is read once,
 * fp64 sums in a fixed order, the arithmetic of the three-launch form) when C % 4 == 0, V <= 1024 and voxels x channels
 * per sample is at most MVD_IN_SMALL_MAX (default 327680: measured at batch 2, profiles/r11_instnorm_small.txt; the backward
 * kernel walks the batch serially, so for N > 2 its limit is 2 / N of that); MVD_IN_SMALL=0 keeps three launches.  mvd_instnorm_single_launch: 1 when the fp32 entry points above would take it -- a producing conv then
 * need not emit tile statistics; mvd_instnorm_single_launches: such launches since the library was loaded. */
int mvd_instnorm_single_launch(long V, int C);
/* launches of the stand-alone forward statistics pass over x (k_in_stats) since the library was loaded */
long mvd_instnorm_stats_pass_launches(void);
long mvd_instnorm_single_launches(void);
/* A/B and test aid: the limit in voxels x channels per sample (0: never; < 0: back to MVD_IN_SMALL_MAX / the default) */
int mvd_set_instnorm_small_max(long max_elems);
/* The launch plan of the InstanceNorm entry points: host arithmetic only (no device call), the function the launch code
 * itself consumes.  dir 0 forward, 1 backward; ntiles > 0: the statistics come from a conv's epilogue tiles; head: the
 * forms of the fused seg head.  Which entry point the arguments describe:
 *   forward   fp32 -> fp32          mvd_instnorm_lrelu_fwd; ntiles > 0: mvd_instnorm_lrelu_fwd_prestats
 *             fp32 / bf16 -> bf16   mvd_instnorm_lrelu_fwd_bf16; bf16 -> bf16 with ntiles > 0: mvd_instnorm_finalize_tiles
 *                                   followed by mvd_instnorm_lrelu_apply_bf16
 *             head                  statistics only: mvd_instnorm_stats_bf16 (y_is_bf16 ignored, C % 4 == 0), ntiles > 0:
 *                                   mvd_instnorm_stats_from_tiles (fp32)
 *   backward  (x, dy) fp32, fp32    mvd_instnorm_lrelu_bwd; head: mvd_instnorm_lrelu_bwd_head
 *             fp32 / bf16, bf16     mvd_instnorm_lrelu_bwd_bf16
 * plan[MVD_IN_PLAN_LEN]: 0 statistics kernel, 1 apply kernel (MVD_IN_* below; the single launch names itself in both),
 * 2 threads, 3 R (voxel rows per block), 4 CG (channel groups per row) of the row-mapped kernels, 5 the block partials per
 * sample the finalize kernel sums, 6 voxels per statistics block (0: the partials come from tiles), 7 / 8 blocks per sample
 * and voxels per block of the apply pass (chunk 0: k_in_apply<1> / k_in_bwd_apply<1>, 256 threads, grid stride), 9 / 10
 * blocks per sample and tiles per block of the tile pass (k_in_finalize_tiles: one wave takes all tiles), 11 / 12 channels
 * and tile rows per 256-thread block of k_in_tiles_reduce.  Returns 2, with a message, for what the entry point refuses
 * by shape or type; the single launch follows mvd_set_instnorm_small_max as the entry points do. */
#define MVD_IN_NONE 0
#define MVD_IN_SMALL_FWD 1       /* k_in_small_fwd */
#define MVD_IN_SMALL_BWD 2       /* k_in_small_bwd */
#define MVD_IN_STATS4 3          /* k_in_stats<4, x type> + k_in_finalize */
#define MVD_IN_STATS1 4          /* k_in_stats<1> + k_in_finalize */
#define MVD_IN_TILES_REDUCE 5    /* k_in_tiles_reduce + k_in_finalize */
#define MVD_IN_FINALIZE_TILES 6  /* k_in_finalize_tiles */
#define MVD_IN_APPLY_ROWS 7      /* k_in_apply_rows<false, y type> */
#define MVD_IN_APPLY1 8          /* k_in_apply<1> */
#define MVD_IN_APPLY_SS16 9      /* k_in_apply_ss16 */
#define MVD_IN_BWD_STATS4 10     /* k_in_bwd_stats<4, x type, dy type> + k_in_bwd_finalize */
#define MVD_IN_BWD_STATS1 11     /* k_in_bwd_stats<1> + k_in_bwd_finalize */
#define MVD_IN_BWD_STATS_HEAD 12 /* k_in_bwd_stats<4, false, false, K> + k_in_bwd_finalize */
#define MVD_IN_BWD_APPLY_ROWS 13 /* k_in_bwd_apply_rows<x type, dy type> */
#define MVD_IN_BWD_APPLY1 14     /* k_in_bwd_apply<1> */
#define MVD_IN_BWD_APPLY_HEAD 15 /* k_in_bwd_apply_rows<false, false, K> */
#define MVD_IN_PLAN_LEN 13
int mvd_instnorm_plan(int dir, int N, long V, int C, int x_is_bf16, int y_is_bf16, long ntiles, int head, long *plan);
/* The same backward for the block whose only consumer is the fused seg head (mvd_seghead_*_fused), from the head's planar
 * logit gradient dlogits [N,K,V] and weight w [K,C]: dy[v][c] = sum_k dlogits[k][v] * w[k][c] is formed inside the two
 * passes (the value mvd_seghead_bwd_fused stores as dx, bit for bit), so that tensor is neither written nor read back --
 * call mvd_seghead_bwd_fused with dx = NULL for dw / dbias.  fp32, C % 4 == 0, K <= 8.  Always the three-launch kernels:
 * results bit-identical to mvd_seghead_bwd_fused + mvd_instnorm_lrelu_bwd in its three-launch form (a volume small enough
 * for that entry's single launch differs from it in the order of the fp64 sums). */
int mvd_instnorm_lrelu_bwd_head(const float *x, const float *dlogits, const float *w, int K, const float *gamma,
                                const float *beta, const float *mean, const float *rstd, float *dx, float *dgamma,
                                float *dbeta, int N, long V, int C, float slope, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * The tail of a residual block (BasicBlockD of ResidualEncoderUNet), fp32, [N,V,C] NDHWC (csrc/resblock.hip):
 *     y = LeakyReLU_slope( IN(a) * gamma_a + beta_a + R )
 * a: the raw output of the block's second conv.  gamma_r == NULL: R = r, a finished tensor (identity skip, pool-only
 * skip).  Otherwise R = IN(r) * gamma_r + beta_r with r the raw output of the 1x1x1 projection of the skip branch, normalised
 * in the same pass (the normalised skip tensor is never written).  mean / rstd [N][C] of a (and of r in the projection form)
 * are outputs, saved for the backward pass; have_stats bit 0 (a) / bit 1 (r): that pair was already filled by the caller
 * (mvd_instnorm_stats_from_tiles on the producing conv's tile statistics) and its statistics pass is skipped.
 * Statistics as the InstanceNorm entries: fp64 partial sums in a fixed order, biased variance, no atomics (results are
 * bit-identical from run to run).  ws: mvd_resblock_workspace_bytes.
 * mvd_resblock_bwd: da, dr [N,V,C], dgamma_a / dbeta_a (and dgamma_r / dbeta_r in the projection form) [C], overwritten.  The
 * LeakyReLU branch is that of the forward pass: z is re-computed from a and r with the forward's arithmetic, z == 0 takes the
 * slope.  dr is the masked gradient itself (identity form) or its InstanceNorm backward through r (projection form);
 * accumulate != 0 adds it into dr instead of overwriting (the block input of the identity form feeds the first conv too).
 * C % 4 == 0 loads four channels at a time under the alignment rule of the InstanceNorm entries (a, r, y, dy, da, dr 16-byte
 * aligned, refused before any launch otherwise); every other C takes a scalar path.  N, V, C <= 0, V == 1 (no variance),
 * N > 65535 and C > 1024 are refused before any launch. */
size_t mvd_resblock_workspace_bytes(int N, long V, int C);
int mvd_resblock_fwd(const float *a, const float *gamma_a, const float *beta_a, const float *r, const float *gamma_r,
                     const float *beta_r, float *y, float *mean_a, float *rstd_a, float *mean_r, float *rstd_r, int N, long V,
                     int C, float eps, float slope, int have_stats, void *ws, size_t ws_bytes, void *stream);
int mvd_resblock_bwd(const float *a, const float *r, const float *dy, const float *gamma_a, const float *beta_a,
                     const float *mean_a, const float *rstd_a, const float *gamma_r, const float *beta_r, const float *mean_r,
                     const float *rstd_r, float *da, float *dr, float *dgamma_a, float *dbeta_a, float *dgamma_r, float *dbeta_r,
                     int accumulate, int N, long V, int C, float slope, void *ws, size_t ws_bytes, void *stream);
/* AvgPool3d(kernel = stride, stride) of the skip branch of a strided residual block, fp32 NDHWC: x [N,D,H,W,C] ->
 * y [N,D/sd,H/sh,W/sw,C], stride 1 or 2 per axis (AvgPool2d on the [N,C,1,H,W] view with stride (1,s,s)).  An odd extent on a
 * strided axis is refused: torch's pool floors where the strided conv beside it does not, so the block cannot run there.
 * mvd_avgpool3d_bwd: dx = dy of the window / window size; accumulate != 0 adds into dx.  D, H, W are the INPUT extents in
 * both calls.  Alignment as above. */
int mvd_avgpool3d_fwd(const float *x, float *y, int N, int D, int H, int W, int C, const int stride[3], void *stream);
int mvd_avgpool3d_bwd(const float *dy, float *dx, int N, int D, int H, int W, int C, const int stride[3], int accumulate,
                      void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * BatchNorm3d(eps, affine, momentum, track_running_stats) + LeakyReLU(slope), fused.  Replaces the nn.BatchNorm3d +
 * nn.LeakyReLU of every ConvDropoutNormReLU of the BN trainer variant
 * (variants/network_architecture/nnUNetTrainerBN.py:31-32: norm_op = get_matching_batchnorm(conv_op), norm_op_kwargs =
 * {'eps': 1e-5, 'affine': True}).  x, y, dy, dx: [N,V,C] NDHWC, fp32 or bf16 storage (x_is_bf16 / y_is_bf16; dy has y's
 * type, dx has x's); gamma, beta, mean, rstd, the running buffers and dgamma / dbeta are fp32 [C].  Statistics over the
 * M = N*V values of a channel: fp64 partial sums per block, one wave per channel sums them in a fixed order (no atomics:
 * bit-identical from run to run).  The library allocates nothing: ws of mvd_batchnorm_workspace_bytes (partials
 * [N][nblk][C][2] doubles, nblk from mvd_batchnorm_nblk, + [C][2] floats).
 *   _fwd (training): mean / rstd (biased variance, eps inside the root) are outputs saved for _bwd; running_mean =
 *     (1-m) running_mean + m mean and running_var = (1-m) running_var + m var M/(M-1) are updated in place and
 *     num_batches_tracked (ONE int64 on the device) is incremented by the finalize kernel, so a replayed graph advances
 *     all three.  M == 1 is refused, as torch refuses it.
 *   _eval: one pass with the running statistics, which it only reads.
 *   _bwd (of _fwd only): dx = gamma rstd (dz - sum dz / M - xhat sum(dz xhat) / M); dgamma / dbeta are overwritten. */
int mvd_batchnorm_nblk(int N, long V, int C);
size_t mvd_batchnorm_workspace_bytes(int N, long V, int C);
int mvd_batchnorm_lrelu_fwd(const void *x, int x_is_bf16, const float *gamma, const float *beta, void *y, int y_is_bf16,
                            float *mean, float *rstd, float *running_mean, float *running_var,
                            int64_t *num_batches_tracked, int N, long V, int C, float eps, double momentum, float slope,
                            void *ws, size_t ws_bytes, void *stream);
int mvd_batchnorm_lrelu_eval(const void *x, int x_is_bf16, const float *gamma, const float *beta, void *y, int y_is_bf16,
                             const float *running_mean, const float *running_var, int N, long V, int C, float eps,
                             float slope, void *stream);
int mvd_batchnorm_lrelu_bwd(const void *x, int x_is_bf16, const void *dy, int y_is_bf16, const float *gamma,
                            const float *beta, const float *mean, const float *rstd, void *dx, float *dgamma, float *dbeta,
                            int N, long V, int C, float slope, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * 1x1x1 segmentation head (K5): x NDHWC [N,V,C] -> logits planar [N,K,V].  Replaces decoder.seg_layers[s]
 * (UNetDecoder.py:70,110).  w: torch layout [K][C], bias [K]. */
int mvd_seghead_fwd(const float *x, const float *w, const float *bias, float *logits, int N, long V, int C, int K,
                    void *stream);
/* dx [N,V,C] (overwritten, or accumulated into when accumulate != 0); dw [K][C], dbias [K] */
size_t mvd_seghead_bwd_workspace_bytes(int N, long V, int C, int K);
int mvd_seghead_bwd(const float *x, const float *w, const float *dlogits, float *dx, float *dw, float *dbias, int N,
                    long V, int C, int K, int accumulate, void *ws, size_t ws_bytes, void *stream);
/* Which kernel the entry points above (fp32 and bf16 alike) run for a shape; no device call.  `aligned`: bit 0 x, bit 1 w,
 * bit 2 dlogits, bit 3 dx lies on a 16-byte boundary.  -1: a shape the entry points refuse (K > 8, ...).
 * fwd: 0 k_seghead_fwd, 1 k_seghead_fwd_vox (C % 4 == 0), 2 / 4 / 8 k_seghead_fwd_voxp<P> (C % 32 == 0, C >= 64, fewer than
 * 2^20 voxels in the batch).  dx: 0 k_seghead_dx, 1 k_seghead_dx4 (C % 4 == 0, C <= 1024, V % 4 == 0).
 * dw: 0 k_seghead_dw, 1 k_seghead_dw4 (C % 4 == 0, C <= 1024), 2 k_seghead_dw4v (V % 4 == 0 as well). */
int mvd_seghead_fwd_path(int N, long V, int C, int K, int aligned);
int mvd_seghead_dx_path(int N, long V, int C, int K, int aligned);
int mvd_seghead_dw_path(int N, long V, int C, int K, int aligned);

/* ------------------------------------------------------------------------------------------------------------
 * Fused softmax + cross-entropy + soft-Dice statistics (K7).  Replaces DC_and_CE_loss
 * (nnUNetTrainer.py:359-361: RobustCrossEntropyLoss + MemoryEfficientSoftDiceLoss{smooth 1e-5, do_bg False}).
 * logits planar [N,K,V]; target float labels [N,V] (robust_ce_loss.py:12-16 casts float->long).
 * fwd: stats[N][3K+1]: per sample (sum p*y, sum p, sum y) for k = 0..K-1, then the sample's sum_vox -log p_target
 * (fp64 accumulation, fixed order, rounded once to fp32).  This is also the tensor that is all-gathered for
 * DDP batch-dice (ddp_allgather.py:25-48, collective C2).
 * mvd_dcce_finalize does the scalar composition (dc = (2I+s)/clip(G+P+s,1e-8); mean over (n, k>=kstart);
 * batch_dice sums over n first) and emits the per-(n,k) Dice gradient coefficients used by bwd.  The Dice part may
 * be evaluated on a different sample set (`dstats`, Nd samples: the all-gathered stats) than the CE part. */
size_t mvd_dcce_workspace_bytes(int N, long V, int K);
int mvd_dcce_fwd(const float *logits, const float *target, float *stats /*[N][3K+1]*/, int N, long V, int K, void *ws,
                 size_t ws_bytes, void *stream);
/* loss[0] = w_ce*CE + w_dice*(-mean dc); loss[1] = CE; loss[2] = -mean dc;
 * coef[Nd][K][2] = w_dice * (dLdice/dI, dLdice/dP) (zero for k < kstart). */
int mvd_dcce_finalize(const float *stats, int N, const float *dstats, int Nd, float *loss, float *coef, long V, int K,
                      int batch_dice, int do_bg, float smooth, float w_ce, float w_dice, void *stream);
/* dlogits[n,k,v] = g * ( w_ce/(N*V) * (p_k - y_k) + p_k * (q_k - sum_j p_j q_j) ),  q_k = coefI[n,k]*y_k + coefP[n,k],
 * g = gscale_host * (gscale_dev ? gscale_dev[0] : 1) */
int mvd_dcce_bwd(const float *logits, const float *target, const float *coef /*[N][K][2]*/, const float *gscale_dev,
                 float gscale_host, float *dlogits, int N, long V, int K, float w_ce, void *stream);
/* p_sel[n,v] = softmax(logits[n,:,v])[sel] (MVDTrainer.py:907 takes channel 2 of the prediction for the topology
 * term; the build feeds the probability to soft-clDice).  bwd: dlogits[n,k,v] = g[n,v] * p_sel * ((k==sel) - p_k). */
int mvd_softmax_select_fwd(const float *logits, float *p_sel, int N, long V, int K, int sel, void *stream);
int mvd_softmax_select_bwd(const float *logits, const float *g, float *dlogits, int N, long V, int K, int sel,
                           void *stream);
/* mask[i] = (labels[i] == value) ? 1.f : 0.f  (one-hot channel `value` of the target, MVDTrainer.py:904-908) */
int mvd_label_mask(const float *labels, float *mask, long n, float value, void *stream);
/* validation: argmax -> one-hot -> tp/fp/fn per class over (n, v) (nnUNetTrainer.py:973-990).  counts[K][3] i64 */
int mvd_argmax_counts(const float *logits, const float *target, long long *counts, int N, long V, int K,
                      void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * KL distillation (K8).  Replaces distill_kl / l2_loss(channel_wise=True) (other_loss.py:51-64, :67-76):
 *   loss = T^2/(N*Ceff*V) * sum p_t * (log p_t - log_softmax(y_s/T + eps_s)),  p_t = softmax(y_t/T) over channels.
 * Element (n,c,v) lives at n*sn + c*sc + v*sv (planar: sc = V, sv = 1; NDHWC: sc = 1, sv = C).
 * pad_zero_channel != 0 implements the C == 1 branch (:55-57): a zero logit channel is appended (Ceff = 2).
 * out[0] = loss.  bwd writes g_s, g_t (either may be NULL) = gscale[0] * dloss/dy. */
size_t mvd_kl_workspace_bytes(int N, long V);
int mvd_kl_fwd(const float *ys, const float *yt, float *out, int N, int C, long V, long sn, long sc, long sv,
               float T, float eps_s, int pad_zero_channel, void *ws, size_t ws_bytes, void *stream);
int mvd_kl_bwd(const float *ys, const float *yt, const float *gscale_dev, float gscale_host, float *gs, float *gt,
               int N, int C, long V, long sn, long sc, long sv, float T, float eps_s, int pad_zero_channel,
               void *stream);
/* bf16 feature maps (mixed precision): dense NDHWC rows [N*V][C], C in {4,8,16,32}, no zero-channel padding; fp32
 * arithmetic, bf16 gradients.  Workspace: mvd_kl_workspace_bytes. */
int mvd_kl_fwd_bf16(const uint16_t *ys, const uint16_t *yt, float *out, int N, int C, long V, float T, float eps_s,
                    void *ws, size_t ws_bytes, void *stream);
int mvd_kl_bwd_bf16(const uint16_t *ys, const uint16_t *yt, const float *gscale_dev, float gscale_host, uint16_t *gs,
                    uint16_t *gt, int N, int C, long V, float T, float eps_s, void *stream);

/* Plain feature MSE: l2_loss(input, target, channel_wise=False) = mean(|a - b|^2) over all n elements
 * (nnunetv2/training/loss/other_loss.py:77-78).  Elementwise: any dense layout, both tensors in the same one.
 * out[0] = loss; bwd writes ga = g[0] * 2 (a - b) / n and gb = -ga (either may be NULL). */
size_t mvd_mse_workspace_bytes(long n);
int mvd_mse_fwd(const float *a, const float *b, float *out, long n, void *ws, size_t ws_bytes, void *stream);
int mvd_mse_bwd(const float *a, const float *b, const float *g_dev, float *ga, float *gb, long n, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Soft skeleton primitives (K9).  Replace soft_erode / soft_dilate of soft_skeleton.py:6-22 on planar volumes
 * [NC, D, H, W].  Bit-exact vs torch CPU (min/max only).  bwd reproduces autograd's routing: max_pool3d sends the
 * gradient to the FIRST maximum in scan order; torch.min(a,b) splits ties 1/2-1/2 (so the three axis pools of
 * erode get 1/4,1/4,1/2 on a triple tie). */
/* `code` (optional in fwd, required by bwd): per-voxel routing record written by fwd (uint16 for erode: arg-min
 * position per axis + tie pattern; uint8 for dilate: arg-max position 0..26 in the 3x3x3 window). */
int mvd_soft_erode_fwd(const float *x, float *y, uint16_t *code, int NC, int D, int H, int W, void *stream);
int mvd_soft_erode_bwd(const uint16_t *code, const float *dy, float *dx, int NC, int D, int H, int W, void *stream);
int mvd_soft_dilate_fwd(const float *x, float *y, uint8_t *code, int NC, int D, int H, int W, void *stream);
int mvd_soft_dilate_bwd(const uint8_t *code, const float *dy, float *dx, int NC, int D, int H, int W, void *stream);
/* skeleton update (soft_skeleton.py:31,35-36): delta = relu(img - opened); init: skel = delta;
 * else skel_out = skel + relu(delta - skel*delta) (no FMA contraction).  n = element count. */
int mvd_skel_update_fwd(const float *img, const float *opened, const float *skel_in, float *skel_out, long n,
                        int init, void *stream);
/* grads: d_img, d_opened (= -d_img masked), d_skel_in (NULL when init) from d_skel_out */
int mvd_skel_update_bwd(const float *img, const float *opened, const float *skel_in, const float *d_skel_out,
                        float *d_img, float *d_opened, float *d_skel_in, long n, int init, void *stream);
/* One whole soft_skel step (soft_skeleton.py:30-31 when init != 0, :33-36 otherwise) in one launch, LDS-tiled:
 *   init:  o = dilate(erode(img));                     skel_out = relu(img - o)
 *   else:  e1 = erode(img); o = dilate(erode(e1));     skel_out = skel_in + relu(d - skel_in * d), d = relu(e1 - o)
 * Writes e1 (the next iteration's img; NULL when init), opened = o (saved for the backward of the update) and, when the
 * pointers are non-NULL, the routing codes of the three stencils in the format of mvd_soft_erode_fwd /
 * mvd_soft_dilate_fwd, so mvd_soft_erode_bwd / mvd_soft_dilate_bwd / mvd_skel_update_bwd back-propagate it.  Bit-exact
 * with the primitive-per-launch chain. */
int mvd_skel_iter_fwd(const float *img, const float *skel_in, float *e1, float *opened, float *skel_out, uint16_t *c_e1,
                      uint16_t *c_e2, uint8_t *c_o, int NC, int D, int H, int W, int init, void *stream);
/* sums for soft-clDice: out[0] = sum a*b, out[1] = sum a  (fixed-order) */
int mvd_dot_sum(const float *a, const float *b, float *out, long n, void *ws, size_t ws_bytes, void *stream);
size_t mvd_dot_sum_workspace_bytes(long n);

/* soft-clDice scalar composition (clDice_metric.py:7-36 formula on soft skeletons):
 * sums = (sum skel_p*tgt, sum skel_p, sum skel_t*pred, sum skel_t); tprec = (s0+smooth)/(s1+smooth),
 * tsens = (s2+smooth)/(s3+smooth); out[0] = 1 - 2*tprec*tsens/(tprec+tsens); out[1..4] = d out[0] / d sums[0..3]. */
int mvd_cldice_combine(const float *sums, float *out, float smooth, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Connected components on a voxel grid (K12; integer, bit-exact).  Replaces the H0 / connected-component step the
 * reference runs on the CPU through the vendored TopologyLayer C++ (hom.cpp:51-69 restricted to vertices+edges
 * == union-find).  mask: uint8 [D,H,W]; labels int32 [D,H,W]: 0 = background, else 1 + smallest linear index of
 * the component (canonical).  conn in {6, 14, 26}.  count[0] = number of components. */
int mvd_cc_label(const uint8_t *mask, int32_t *labels, int32_t *count, int D, int H, int W, int conn, void *stream);
/* mask[v] = (f[v] > thr) (or >= when ge != 0) */
int mvd_threshold_mask(const float *f, uint8_t *mask, long n, float thr, int ge, void *stream);

/* H0 persistence: birth / death pairing of the connected components of the sub- (sublevel != 0) or super-level sets
 * of a scalar field f [D,H,W] on the grid graph with conn in {6, 14 (Freudenthal), 26}.  Replaces, for maxdim 0, the
 * CPU persistence of the vendored TopologyLayer C++: lower-star extension complex.cpp:136-146, filtration order
 * complex.cpp:182-196, reduction hom.cpp:51-69 (== union-find with the elder rule on vertices + edges), one bar per
 * vertex hom.cpp:155-185, called from functional/sublevel.py:21-49 / nn/levelset.py:137-163 after a D2H copy.
 *   device (mvd_h0_sorted_edges): keys_sorted[e] = all D*H*W*n_off 64-bit edge keys, ascending:
 *       (order-preserving bits of max(g[u], g[v])) << 32 | (v * n_off + k), g = f or -f; edges that leave the grid
 *       carry ~0 and sort last; the first mvd_h0_num_edges() keys are the filtration order of the 1-cells.
 *   host (mvd_h0_pair_host, plain C++): one elder-rule union-find sweep over those keys copied to host memory.
 *       death[v] / death_vertex[v] describe the bar born at vertex v (birth value f[v]): the value at which it dies
 *       (+inf, resp. -inf for super-level, for the essential bar of each component) and the critical (arg-max) vertex
 *       of the killing edge (-1 for essential bars) -- the `backprop_lookup` of hom.cpp:178-183.  Returns the number
 *       of essential bars, < 0 on error.
 * Integer / comparison work: bit-exact against oracle/cc_oracle.c, multiset-exact against the reference C++. */
long mvd_h0_num_edges(int D, int H, int W, int conn);
size_t mvd_h0_workspace_bytes(int D, int H, int W, int conn);
int mvd_h0_sorted_edges(const float *f, uint64_t *keys_sorted, int D, int H, int W, int conn, int sublevel, void *ws,
                        size_t ws_bytes, void *stream);
long mvd_h0_pair_host(const float *f_host, const uint64_t *keys_host, long n_edges, int D, int H, int W, int conn,
                      int sublevel, float *death, int64_t *death_vertex);

/* Connected-component post-processing of a predicted segmentation.  Replaces, on device,
 * remove_all_but_largest_component_from_segmentation (nnunetv2/postprocessing/remove_connected_components.py:22-34):
 *   mask = union over label_set of (seg == l)            -> mvd_seg_label_mask  (region_or_label_to_mask, :27-30)
 *   cc   = mvd_cc_label(mask, conn = 26)                  (skimage.measure.label full connectivity inside acvl_utils)
 *   kept = the `keep` (1 or 2) largest components         -> mvd_cc_keep_largest (remove_all_but_two_largest_component, :31)
 *   out  = seg, with mask & ~kept set to background       -> mvd_seg_remove_components (:32-33)
 * All integer; bit-exact against oracle/postproc_oracle.py.  Ties in component size go to the component with the
 * smaller canonical label (first in scan order).  label_set is a HOST array of 1..16 labels.  kept: int32[4] on the
 * device = {label0, label1, size0, size1} (0 = none).  workspace: mvd_cc_keep_workspace_bytes(n) device bytes. */
int mvd_seg_label_mask(const int32_t *seg, uint8_t *mask, long n, const int32_t *label_set, int nlabels, void *stream);
/* sizes int32[n]: sizes[root] = voxel count of the component whose canonical label is root + 1, 0 everywhere else (the
 * size pass of mvd_cc_keep_largest on its own; integer atomics, exact). */
int mvd_cc_component_sizes(const int32_t *cc_labels, int32_t *sizes, long n, void *stream);
size_t mvd_cc_keep_workspace_bytes(long n);
int mvd_cc_keep_largest(const int32_t *cc_labels, long n, int keep, int32_t *kept, void *workspace, void *stream);
int mvd_seg_remove_components(const int32_t *seg, const int32_t *cc_labels, const int32_t *kept, int32_t *out, long n,
                              int background, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * SGD(momentum, nesterov, weight decay) with global-norm clipping (K10).  Replaces
 * torch.nn.utils.clip_grad_norm_(params, 12) + torch.optim.SGD.step (nnUNetTrainer.py:473-477, :918-924) on flat
 * parameter / gradient / momentum buffers of n floats.
 *   sumsq: out[0] = sum g^2 (fixed-order).  step: g *= grad_scale (1/world_size under data parallelism: the mean
 *   DDP takes after its SUM all-reduce, nnUNetTrainer.py:220-222; 1 otherwise); g *= min(1, max_norm /
 *   (grad_scale*sqrt(sumsq)+1e-6)) (read from device memory: no host sync); g += wd*p; buf = first ? g : mom*buf + g;
 *   g = g + mom*buf (nesterov); p -= lr*g */
size_t mvd_sumsq_workspace_bytes(long n);
int mvd_grad_sumsq(const float *g, float *out, long n, void *ws, size_t ws_bytes, void *stream);
int mvd_sgd_nesterov_step(float *p, const float *g, float *buf, const float *sumsq, long n, float lr, float momentum,
                          float weight_decay, float max_norm, float grad_scale, int first_step, void *stream);
/* the same step with its scalars read from a DEVICE array hyper[6] = {lr, momentum, weight_decay, max_norm, grad_scale,
 * first_step (0/1)}: a hipGraph-captured train step (nnUNetTrainer.py:888-925 replayed as one graph launch) follows the
 * PolyLR schedule (polylr.py:16-20, stepped per epoch :880) without re-capture.  sumsq must be given (max_norm <= 0 in
 * hyper[3] switches clipping off). */
int mvd_sgd_nesterov_step_dev(float *p, const float *g, float *buf, const float *sumsq, long n, const float *hyper,
                              void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Adam / AdamW (optionally amsgrad) with global-norm clipping.  Replaces torch.nn.utils.clip_grad_norm_(params, 12) +
 * torch.optim.Adam(W).step (variants/optimizer/nnUNetTrainerAdam.py:10-13, :22-24) on flat parameter / gradient /
 * exp_avg / exp_avg_sq [/ max_exp_avg_sq] buffers of n floats; sumsq comes from mvd_grad_sumsq.  vmax == NULL: amsgrad
 * off.  decoupled != 0: AdamW (p *= 1 - lr*wd), else Adam (g += wd*p).
 *   hyper: DEVICE buffer of 128 bytes, 8-byte aligned: 8 doubles written by the caller {lr, beta1, beta2, eps,
 *     weight_decay, max_norm (<= 0: no clipping), grad_scale, unused}, then 16 floats the library writes.
 *   step:  DEVICE int64, the number of steps taken so far (0 before the first).
 * Two launches on `stream`: one thread sets step += 1 and forms the fp32 scalars of the update (lr / (1 - beta1^step),
 * sqrt(1 - beta2^step), 1 - lr*wd, ...) in fp64 behind hyper's doubles; the streaming kernel reads only those, so a
 * hipGraph-captured step follows the schedule and the bias correction without re-capture.
 *   g *= grad_scale; g *= min(1, max_norm / (grad_scale*sqrt(sumsq)+1e-6)); weight decay; m += (1-beta1)*(g-m);
 *   v = v*beta2 + (1-beta2)*g*g; vhat = amsgrad ? (vmax = max(vmax, v)) : v;
 *   p -= step_size*m / (sqrt(vhat)/bc2sqrt + eps) */
int mvd_adam_step(float *p, const float *g, float *m, float *v, float *vmax, const float *sumsq, long n, double *hyper,
                  long long *step, int decoupled, void *stream);

/* misc elementwise helpers used by the host glue (all fixed-order / exact) */
int mvd_nchw_to_ndhwc(const float *src, float *dst, int N, int C, long V, void *stream);
int mvd_ndhwc_to_nchw(const float *src, float *dst, int N, int C, long V, void *stream);
/* bf16 mixed precision, narrow network input (4 modalities): fp32 [N][C][V] (src_ndhwc = 0) or [N][V][C] -> bf16
 * [N][V][Cpad] with zero channels C .. Cpad-1 (C <= 8, Cpad = 32), so that the first conv runs on the 32-channel bf16
 * engines (get_network_from_plans.py:41-44 under the autocast of nnUNetTrainer.py:906: bf16 operands, fp32 accumulate). */
int mvd_pad_channels_bf16(const float *src, uint16_t *dst, int N, int C, int Cpad, long V, int src_ndhwc, void *stream);
int mvd_axpy(float *y, const float *x, float a, long n, void *stream); /* y += a*x */

/* ------------------------------------------------------------------------------------------------------------
 * Sliding-window inference helpers.  Planar fp32 [C][D][H][W].
 * mvd_flip_add: dst (+)= flip(src) on the axes of mask (bit 0: D, 1: H, 2: W) -- the mirror test-time augmentation of
 *   predict_from_raw_data.py:562-588 (torch.flip of the input and of each prediction, summed);
 * mvd_sw_accumulate: logits[:, tile] += tile_logits * scale * gauss, npred[tile] += gauss (gauss NULL: weight 1)
 *   -- predict_from_raw_data.py:706-707;  mvd_sw_normalize: logits /= npred (:709). */
int mvd_flip_add(const float *src, float *dst, int C, int D, int H, int W, int mask, int accumulate, void *stream);
int mvd_sw_accumulate(const float *tile, const float *gauss, float scale, float *logits, float *npred, int K, int pd, int ph,
                      int pw, int D, int H, int W, int oz, int oy, int ox, void *stream);
int mvd_sw_normalize(float *logits, const float *npred, int K, long V, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * On-device training feed (the deterministic part).  Replaces, for case volumes resident in HBM, the
 * crop + constant pad of nnUNetDataLoader3D.generate_train_batch (dataloading/data_loader_3d.py:31-46: data padded
 * with 0, seg with -1), MirrorTransform (nnUNetTrainer.py:738-739), RemoveLabelTransform(-1, 0) (:745) and
 * DownsampleSegForDSTransform2 order 0 (deep_supervision_donwsampling.py:27-55) + NumpyToTensor 'float' (:768).
 * Planar layouts: vol/seg [C][D][H][W] of one case; out [C][pd][ph][pw] float32 (the caller offsets `out` to batch
 * row j).  (lbz, lby, lbx) = bbox_lbs of get_bbox (base_data_loader.py:56-139; may be negative / overhang).
 * flip_mask bit 0/1/2 mirrors D/H/W of the padded patch.  Bit-exact against oracle/feed_oracle.py. */
int mvd_feed_crop_pad_f32(const float *vol, float *out, int C, int D, int H, int W, int pd, int ph, int pw, int lbz,
                          int lby, int lbx, int flip_mask, float pad, void *stream);
/* int16 segmentation -> float32 target; after padding with `pad`, voxels equal to replace_from become replace_to
 * when `replace` != 0 */
int mvd_feed_crop_pad_seg_i16(const int16_t *seg, float *out, int C, int D, int H, int W, int pd, int ph, int pw, int lbz,
                              int lby, int lbx, int flip_mask, int pad, int replace, int replace_from, int replace_to,
                              void *stream);
/* order-0 resize [BC][D][H][W] -> [BC][d][h][w]: source index floor((2o+1)n/(2m)) per axis (pixel-centre aligned
 * nearest neighbour == skimage.transform.resize(order=0) == scipy.ndimage.zoom(order=0, grid_mode=True)) */
int mvd_feed_downsample_seg(const float *in, float *out, long BC, int D, int H, int W, int d, int h, int w, void *stream);

/* SpatialTransform of the feed (nnUNetTrainer.py:703-714: batchgenerators augment_spatial, rotation + scaling, order 3
 * data / order 1 seg, border mode 'constant'), on the initial patch [C][D][H][W] cut by mvd_feed_crop_pad_* (data pad 0,
 * seg pad -1).  Pinned to scipy.ndimage.
 * mvd_feed_bspline_prefilter_f32: in place, spline_filter1d(order=3, mode='mirror') along the axes of axis_mask (bit 0:
 *   D, 1: H, 2: W; W <= 16383), all C channels per launch; a length-1 axis is left unchanged.
 * mvd_feed_warp_data_f32: out[C][fd][fh][fw] = map_coordinates(coef, p, order=3, mode='constant', cval) with coef the
 *   prefiltered patch and p(o) = A (o - (f-1)/2) + off; affine12 is a HOST array {A row-major (9), off (3)} copied into
 *   the kernel arguments (no device copy: the call is capturable).  flip_mask mirrors the OUTPUT (MirrorTransform).
 * mvd_feed_warp_seg: the same p with 8 linear taps: out = the largest label whose indicator reaches 0.5, 0 where none
 *   does and outside [0, n-1] (interpolate_img(order=1, cval=-1, is_seg=True)); then replace_from -> replace_to when
 *   `replace` != 0 (RemoveLabelTransform(-1, 0)).  seg holds integer labels as float32. */
int mvd_feed_bspline_prefilter_f32(float *x, int C, int D, int H, int W, int axis_mask, void *stream);
int mvd_feed_warp_data_f32(const float *coef, float *out, int C, int D, int H, int W, int fd, int fh, int fw,
                           const double *affine12, int flip_mask, float cval, void *stream);
int mvd_feed_warp_seg(const float *seg, float *out, int C, int D, int H, int W, int fd, int fh, int fw,
                      const double *affine12, int flip_mask, int replace, int replace_from, int replace_to,
                      void *stream);

/* The in-plane ("dummy 2-D") form of the same transform for anisotropic plans (nnUNetTrainer.py:695-717,
 * Convert3DTo2DTransform / Convert2DTo3DTransform around the SpatialTransform): [C][D][H][W] is resampled as
 * C*D independent slices under ONE in-plane map p(oy, ox) = A (o - (f-1)/2) + off, o = (oy, ox), f = (fh, fw); axis 0
 * keeps its size D.  affine6 is a HOST array {A row-major 2x2 (4), off (2)} copied into the kernel arguments.  Pinned
 * to scipy.ndimage per slice.  coef is prefiltered in-plane only (mvd_feed_bspline_prefilter_f32 with axis_mask 6).
 * H*W < 2^31, C*D < 8*65535.
 * mvd_feed_warp2d_data_f32: out[C][D][fh][fw] = 2-D map_coordinates(coef[c][z], p, order=3, mode='constant', cval), 16
 *   taps.  flip_mask is still the 3-bit OUTPUT mirror: bit 0 flips the slice index z, bits 1 / 2 the in-plane axes.
 * mvd_feed_warp2d_seg: the same p with 4 linear taps and the winner rule and replacement of mvd_feed_warp_seg. */
int mvd_feed_warp2d_data_f32(const float *coef, float *out, int C, int D, int H, int W, int fh, int fw,
                             const double *affine6, int flip_mask, float cval, void *stream);
int mvd_feed_warp2d_seg(const float *seg, float *out, int C, int D, int H, int W, int fh, int fw, const double *affine6,
                        int flip_mask, int replace, int replace_from, int replace_to, void *stream);

/* Intensity augmentations of the feed (nnUNetTrainer.py:719-736: GaussianNoise, GaussianBlur, BrightnessMultiplicative,
 * ContrastAugmentation, SimulateLowResolution, Gamma (inverted), Gamma) and MaskTransform, on the batch patch
 * [C][D][H][W] (V = D*H*W voxels per channel, C <= 16, bit c of chmask selects channel c).  Per-channel parameters are
 * HOST arrays of C values copied into the kernel arguments (capturable calls); statistics stay on the device.  Pinned
 * to numpy / scipy.ndimage.
 * mvd_feed_channel_stats_f32: stats[c] = {mean, std (ddof 0), min, max} (fp64) of channel c, fixed-order two-level
 *   reduction through ws (mvd_feed_stats_workspace_bytes(C)); pre_op 2 / 3 takes them of the gamma map y of x / of -x
 *   (params: gamma per channel, pre_stats: the channel's own stats).
 * mvd_feed_intensity_apply_f32: in place, op 0 x *= p[c]; 1 clip((x - mean) p[c] + mean, min, max) (stats_a);
 *   2 / 3 augment_gamma(retain_stats=True) with gamma p[c] on x / on -x (stats_a of x, stats_b of y); 4 clip(x, min,
 *   max) of stats_a.
 * mvd_feed_gaussian_blur_f32: in place, gaussian_filter(x[c], sigma[c]) (mode 'reflect', truncate 4, sigma <= 1.1) for
 *   every channel with sigma[c] > 0; ws: 2 * (selected channels) * V floats.
 * mvd_feed_gaussian_noise_f32: x[k] += sigma * N(raw_k), k = c V + v the stored voxel, raw_k the k-th output of
 *   numpy.random.Philox(key=key0 + 2^64 key1).random_raw(); N: u1 = (2 (raw >> 41) + 1) 2^-24,
 *   u2 = (2 ((raw >> 18) & (2^23 - 1)) + 1) 2^-24, sqrt(-2 ln u1) cos(2 pi u2).
 * mvd_feed_lowres_gather_f32: dpad [td+2pad][th+2pad][tw+2pad] = zoom(x', (td,th,tw)/(D,H,W), order=0, mode='nearest',
 *   grid_mode=True) edge-padded by pad, with x' the single channel x un-mirrored on flip_mask (SimulateLowResolution's
 *   downsample; the upsample is mvd_feed_bspline_prefilter_f32 + mvd_feed_warp_data_f32 with a diagonal affine).
 * mvd_feed_lowres_gather2d_f32: the in-plane form (ignore_axes=(0,), the dummy 2-D mode): dpad [D][th+2pad][tw+2pad],
 *   axis 0 is neither resized nor padded (bit 0 of flip_mask still un-mirrors its index); the upsample is
 *   mvd_feed_bspline_prefilter_f32 with axis_mask 6 + mvd_feed_warp2d_data_f32 with a diagonal affine.
 * mvd_feed_mask_remove_label: data[c] = 0 where seg[0] < 0 for the channels of chmask (MaskTransform), then
 *   replace_from -> replace_to in all Cs seg channels when `replace` != 0 (RemoveLabelTransform). */
size_t mvd_feed_stats_workspace_bytes(int C);
int mvd_feed_channel_stats_f32(const float *x, double *stats, double *ws, int C, long V, int chmask, int pre_op,
                               const float *params, const double *pre_stats, void *stream);
int mvd_feed_intensity_apply_f32(float *x, int C, long V, int chmask, int op, const float *params,
                                 const double *stats_a, const double *stats_b, void *stream);
int mvd_feed_gaussian_blur_f32(float *x, float *ws, int C, int D, int H, int W, const double *sigma, void *stream);
int mvd_feed_gaussian_noise_f32(float *x, int C, long V, int chmask, uint64_t key0, uint64_t key1, float sigma,
                                void *stream);
int mvd_feed_lowres_gather_f32(const float *x, float *dpad, int D, int H, int W, int td, int th, int tw, int pad,
                               int flip_mask, void *stream);
int mvd_feed_lowres_gather2d_f32(const float *x, float *dpad, int D, int H, int W, int th, int tw, int pad,
                                 int flip_mask, void *stream);
int mvd_feed_mask_remove_label(float *data, float *seg, int C, int Cs, long V, int chmask, int replace,
                               int replace_from, int replace_to, void *stream);

/* The DA5 recipe of the feed (variants/data_augmentation/nnUNetTrainerDA5.py: MedianFilter, Sharpening, the two
 * LocalTransforms, BlankRectangle, Rot90 / TransposeAxes / Mirror, the wider GaussianBlur, additive Brightness and the
 * unclipped Contrast) on the batch patch [C][D][H][W], C <= 16.  Per-channel parameters are HOST arrays copied
 * into the kernel arguments; statistics ({mean, std, min, max} per channel, mvd_feed_channel_stats_f32) stay on the
 * device.  No float atomics: results are bit-identical from run to run.  Inputs are finite (NaN is unsupported).
 * mvd_feed_median_filter_f32: out[c] = scipy.ndimage.median_filter(x[c], size=sizes[c]) (mode 'reflect'), sizes 2..7:
 *   the element of rank s^3 / 2 of the window i - s/2 .. i + (s-1) - s/2 per axis, exactly; sizes[c] == 0 copies the
 *   channel.  out != x.
 * mvd_feed_sharpen_f32: in place, clip(scipy.signal.convolve(x[c], strength[c] L + delta, 'same'), min, max) with L the
 *   3x3x3 filter 6 at the centre, -1 at the six face neighbours, zero border, min / max of the channel from stats;
 *   strength[c] == 0 skips the channel.  ws: C * V floats.
 * mvd_feed_local_gauss_f32: in place on the channels of chmask with g = prod_d exp(-(i_d - loc[c][d])^2 /
 *   (2 scale[c][d]^2)) / max g over the grid: mode 0 x += amount[c] g; mode 1 x01 = (x - mn) / max(mx - mn, 1e-8),
 *   x = x01 ^ (1 + (amount[c] - 1) g) (mx - mn) + mn with mn, mx from stats (mode 0 takes stats == NULL).
 * mvd_feed_blank_rectangle_f32: the box lb .. lb + size of channel c becomes its own mean (fp64 sum in a fixed order,
 *   rounded once).  ws: 64 doubles on the device.
 * mvd_feed_signed_permute_f32: out = flip(transpose(in, perm), flip_mask) over the spatial axes of every channel (any
 *   C <= 4096); permuted axes must have equal extents.  out != in.
 * mvd_feed_gaussian_blur_wide_f32: mvd_feed_gaussian_blur_f32 for sigma <= 1.5 (radius <= 6), the same arithmetic.
 * mvd_feed_da5_apply_f32: in place, op 0 x += p[c]; op 1 (x - mean) p[c] + mean (ContrastAugmentation with
 *   preserve_range=False; stats). */
int mvd_feed_median_filter_f32(const float *x, float *out, int C, int D, int H, int W, const int *sizes, void *stream);
int mvd_feed_sharpen_f32(float *x, float *ws, int C, int D, int H, int W, const double *strength, const double *stats,
                         void *stream);
int mvd_feed_local_gauss_f32(float *x, int C, int D, int H, int W, int chmask, int mode, const double *loc,
                             const double *scale, const float *amount, const double *stats, void *stream);
int mvd_feed_blank_rectangle_f32(float *x, int C, int D, int H, int W, int c, const int *lb, const int *size, double *ws,
                                 void *stream);
int mvd_feed_signed_permute_f32(const float *in, float *out, int C, int D, int H, int W, const int *perm, int flip_mask,
                                void *stream);
int mvd_feed_gaussian_blur_wide_f32(float *x, float *ws, int C, int D, int H, int W, const double *sigma, void *stream);
int mvd_feed_da5_apply_f32(float *x, int C, long V, int chmask, int op, const float *params, const double *stats,
                           void *stream);

/* Cascade stage of the feed (nnUNetTrainer.py:740-755, custom_transforms/cascade_transforms.py) on the
 * one-hot channels of the previous stage's segmentation.  Planes are [D][H][W] float 0/1 (n = D*H*W voxels) or bit-planes
 * [D][H][Wq] of 64-bit words, Wq = ceil(W/64), bit b of word q = voxel x = 64 q + b, pad bits 0
 * (mvd_feed_cascade_plane_words(D,H,W) words per plane).  Label lists and element tables are HOST arrays copied into
 * the kernel arguments (capturable calls).  Bit-exact against scipy.ndimage.
 * mvd_feed_cascade_onehot: out[k][v] = (seg[v] == labels[k]) for the K <= 8 labels (MoveSegAsOneHotToData).
 * mvd_feed_cascade_pack / _unpack: K float planes (non-zero = set) <-> K bit-planes.
 * mvd_feed_cascade_morph: op 0 binary_dilation, 1 binary_erosion(border_value=True), 2 closing (dilation, erosion),
 *   3 opening (erosion, dilation) of bit-plane c of the K planes with the element given as `nrows` <= 256 rows
 *   {dz, dy, lo, hi}: the erosion reads in[z+dz][y+dy][x+lo .. x+hi] (scipy: offset = index - n/2), the dilation the
 *   negated offsets; all offsets within +-8.  Outside the volume is 0 for the dilation, 1 for the erosion.  Then every
 *   other plane loses the voxels the operator added, other &= ~(res & ~before).  tmp: 2 planes of scratch.
 * mvd_feed_cascade_remove: RemoveRandomConnectedComponentFromOneHotEncodingTransform on the float plane chan: label its
 *   26-connected components, call a component valid when its voxel count is < threshold, and clear valid component
 *   number floor(u n_valid) in the order of the components' smallest linear index (scipy.ndimage.label's order); when
 *   `other` is not NULL the same voxels are set to 1 there.  n_valid == 0: nothing changes.  chosen: int32[2] on the
 *   device = {1 + smallest linear index of the removed component or 0, n_valid}.  Fixed-order counts: two runs give
 *   the same bits.  ws: mvd_feed_cascade_remove_workspace_bytes(n) device bytes. */
int mvd_feed_cascade_onehot(const float *seg, float *out, long n, const int *labels, int K, void *stream);
size_t mvd_feed_cascade_plane_words(int D, int H, int W);
int mvd_feed_cascade_pack(const float *planes, uint64_t *bits, int K, int D, int H, int W, void *stream);
int mvd_feed_cascade_unpack(const uint64_t *bits, float *planes, int K, int D, int H, int W, void *stream);
int mvd_feed_cascade_morph(uint64_t *planes, uint64_t *tmp, int K, int c, int op, int D, int H, int W, const int *rows,
                           int nrows, void *stream);
size_t mvd_feed_cascade_remove_workspace_bytes(long n);
int mvd_feed_cascade_remove(float *chan, float *other, int D, int H, int W, long threshold, double u, void *ws,
                            size_t ws_bytes, int32_t *chosen, void *stream);

/* Segmentation export and evaluation after sliding-window inference (the tail of perform_actual_validation,
 * nnUNetTrainer.py:1135-1260).  logits: float [K][d][h][w] in network space.  The resampled size (D,H,W), the
 * pre-crop volume `full`, the lower bbox corner `lo` (HOST int[3] each) are per NETWORK axis; perm = transpose_backward
 * (HOST int[3]): output axis j holds network axis perm[j], and the output is the contiguous volume of extents
 * full[perm[0..2]].  Per-axis interpolation comes as three DEVICE tables of D + H + W entries (axis D first): value =
 * lerp(x[idx0], x[idx1], weight), evaluated with fp32 fmaf along W, then H, then D.  A linear axis (order 1) has
 * c = clamp((o + 0.5) n_in / n_out - 0.5, 0, n_in - 1), idx0 = floor(c), idx1 = min(idx0 + 1, n_in - 1), weight = c - idx0;
 * a nearest axis (order 0, the separate-z axis) idx0 = idx1 = clamp(floor(c + 0.5), 0, n_in - 1), weight 0; an axis of
 * unchanged size is the identity.  Pinned to scipy.ndimage.zoom(order=1, mode='nearest', grid_mode=True) and
 * map_coordinates(order=0, mode='nearest').  Indices are clamped to the logits' extent again in the kernel.
 * mvd_export_resize_argmax_u8: out = uint8 label volume (K <= 255): argmax over the K interpolated channels, the lowest
 *   index on an exact tie, 0 outside the bbox; every output byte is written once, the K x (D,H,W) floats never exist.
 * mvd_export_resize_softmax_f32: out = float [K] planes of the same volume; apply_softmax != 0: fp32 softmax over K,
 *   outside the bbox plane 0 is 1 and the others 0 (label_handling.py:199-205); == 0: the interpolated logits, 0 outside.
 * mvd_seg_confusion_counts: counts[r] = {TP, FP, FN, TN} (int64, device) of label set r (label_sets: HOST int32 [R][16],
 *   set_sizes: HOST int [R], 1..16 labels of 0..255 each, R <= 32) between pred (uint8) and gt (uint8, or int16 when
 *   gt_is_i16), over the voxels whose gt is not ignore_label (when has_ignore).  Integer sums: exact and run-to-run
 *   identical.  Both volumes 16-byte aligned. */
int mvd_export_resize_argmax_u8(const float *logits, unsigned char *out, const int *idx0, const int *idx1,
                                const float *weight, int K, int d, int h, int w, int D, int H, int W, const int *full,
                                const int *lo, const int *perm, void *stream);
int mvd_export_resize_softmax_f32(const float *logits, float *out, const int *idx0, const int *idx1, const float *weight,
                                  int K, int d, int h, int w, int D, int H, int W, const int *full, const int *lo,
                                  const int *perm, int apply_softmax, void *stream);
int mvd_seg_confusion_counts(const unsigned char *pred, const void *gt, int gt_is_i16, long n, const int32_t *label_sets,
                             const int *set_sizes, int R, int has_ignore, int ignore_label, long long *counts,
                             void *stream);

/* Surface distances of two segmentations: medpy's __surface_distances, as evaluation/Hausdorff.py and
 * evaluation/metrics.py:312-382 of the reference use it.  Volumes are [D][H][W], every extent 1..1024.
 * mvd_surf_border: masks A = {a in label_set}, B = {b in label_set} (a, b: uint8, or int16 when *_is_i16; label_set: HOST,
 *   1..16 labels of 0..255).  border[v] bit 0 / bit 1: v belongs to A / B and one of its footprint neighbours
 *   (|dz| + |dy| + |dx| <= connectivity, 1..3) is 0 or lies outside the volume (scipy's binary_erosion, border_value 0).
 *   stats: DEVICE int32[10] = {|A|, |B|, |border A|, |border B|, 1024 - min z, 1024 - min y, 1024 - min x, max z + 1,
 *   max y + 1, max x + 1} with the extrema over the union of A and B (all 0 when both are empty).  Integer atomics.
 * mvd_edt_squared: exact squared Euclidean distance of every voxel of `box` (HOST int[6]: lower corner z, y, x, then
 *   extents) to the nearest site INSIDE the box; a site is a voxel with (vol[v] & bit) != 0, or == 0 when zero_is_site.
 *   spacing == NULL: int32 squared voxel distance (INT32_MAX when the box holds no site); spacing = HOST double[3]: fp64
 *   ((dx sx)^2 + (dy sy)^2) + (dz sz)^2 (+inf without a site).  The result, contiguous over the box, is left at the
 *   START of `workspace` (mvd_edt_workspace_bytes(box extents, spaced) device bytes, 16-byte aligned).
 * mvd_edt_root: out[i] = correctly rounded fp64 root of sq[i] (int32, or double when spaced), +inf for "no site".
 * mvd_surf_gather: the roots at the box voxels whose border byte has `bit`, compacted into out[0 .. capacity) in an
 *   UNSPECIFIED order (slots from an integer counter, DEVICE int32, which ends as the number of such voxels).
 * mvd_surf_reduce: out (DEVICE double[6]) = {sum s0, sum s1, s0[n0 - 1], s1[n1 - 1], all[lo], all[hi]}; the sums are
 *   formed in a fixed order by one block: bit-identical from run to run for identical input. */
int mvd_surf_border(const void *a, int a_is_i16, const void *b, int b_is_i16, int D, int H, int W,
                    const int32_t *label_set, int nlabels, int connectivity, unsigned char *border, int32_t *stats,
                    void *stream);
size_t mvd_edt_workspace_bytes(int bd, int bh, int bw, int spaced);
int mvd_edt_squared(const unsigned char *vol, int bit, int zero_is_site, int D, int H, int W, const int *box,
                    const double *spacing, void *workspace, size_t workspace_bytes, void *stream);
int mvd_edt_root(const void *sq, int spaced, long n, double *out, void *stream);
int mvd_surf_gather(const void *sq, int spaced, const unsigned char *border, int bit, int D, int H, int W, const int *box,
                    double *out, int capacity, int32_t *counter, void *stream);
int mvd_surf_reduce(const double *s0, int n0, const double *s1, int n1, const double *all, int lo, int hi, double *out,
                    void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Region-based training and the ignore label (csrc/loss_region.hip).
 * Region loss = DC_and_BCE_loss({}, {batch_dice, do_bg, smooth, ddp}, use_ignore_label) of upstream nnU-Net 2.1.1 (the
 * class is missing from the fork: parity unpinned, pinned to torch.nn.functional in fp64 by tests/region_loss_ref.py).
 * logits planar [N,R,V], R <= 8 sigmoid heads.  Targets, `target_form`:
 *   0  label map float [N,V] + lut (HOST uint32[256]): bit r of lut[label] = the label belongs to region r, bit 31 = the
 *      label is the ignore label (the mvd_seg_label_mask convention).  Labels truncate like .long(), clamped to 0..255.
 *   1  planes float [N,R,V] (ConvertSegmentationToRegionsTransform's output), a value >= 0.5 is a member voxel; lut unused.
 *   2  planes float [N,R+1,V], the ignore plane last.
 * With m = 1 on the voxels that are not ignored: stats[N][3R+2] = per head (sum m s y, sum m s, sum m y), s = sigmoid(z),
 * then sum m * sum_r bce_r with bce = max(z,0) - z y + log1p(exp(-|z|)) (fp32), then sum m.  fp64 accumulation in a fixed
 * order, no float atomics: run-to-run bit-identical, and forms 0 and 1/2 give identical bits for equivalent targets.
 * The sums are rounded once to the fp32 stats (the mvd_dcce_fwd convention), so sum m y and the valid-voxel count sum m --
 * from which the BCE / CE denominator c is formed -- are exact integers only up to 2^24 voxels per sample (256^3); beyond
 * that they carry fp32's relative error of 6e-8, as torch's own fp32 mask.sum() does.
 * finalize: dc = (2I+s)/clip(G+P+s,1e-8) as mvd_dcce_finalize; BCE = sum / (N R V) without the ignore label and sum /
 * clip(sum m, 1e-8) with it (voxels, not voxels x heads: upstream's own normalisation).  loss[4] = {w_ce*BCE + w_dice*dice,
 * BCE, dice, c} where c is the factor of the backward; coef[Nd][R][2] as mvd_dcce_finalize.
 * bwd: dlogits[n,r,v] = m ? g * ( w_ce c (s - y) + s (1 - s) (coefI[n,r] y + coefP[n,r]) ) : 0 (an exact zero).
 *
 * mvd_dcce_masked_*: DC_and_CE_loss(ignore_label = L) for softmax heads: m = (t != L), the Dice target has L -> 0, I, P, G
 * masked by m, CE = cross_entropy(ignore_index = L) = sum / sum m, and 0 when no voxel is valid (decided on the device).
 * stats[N][3K+2], loss[4] and coef as above; the gradient is mvd_dcce_bwd's with m applied and 1/(N V) replaced by c.
 *
 * Online evaluation (nnUNetTrainer.py:969-1002), int64 counts[R or K][3] = (tp, fp, fn), integer sums, exact:
 * mvd_sigmoid_counts: head r predicts a voxel iff z_r > 0, over m.  "sigmoid(z) > 0.5" is decided as z > 0 everywhere in
 *   this library: exact in real arithmetic; torch's fp32 sigmoid rounds 0 < z < ~1.2e-7 to exactly 0.5 and so calls those
 *   voxels "off".  A logit of exactly 0 is "off" under both.
 * mvd_argmax_counts_masked: mvd_argmax_counts over m, the target's L counted nowhere.
 * mvd_seg_to_regions: planes float [N,R(+1),V] of a label map (region_based_training.py:23-38; the ignore plane last). */
size_t mvd_dcbce_workspace_bytes(int N, long V, int R);
int mvd_dcbce_fwd(const float *logits, const float *target, int target_form, const uint32_t *lut_host, float *stats, int N,
                  long V, int R, void *ws, size_t ws_bytes, void *stream);
int mvd_dcbce_finalize(const float *stats, int N, const float *dstats, int Nd, float *loss, float *coef, long V, int R,
                       int batch_dice, int do_bg, int use_ignore_label, float smooth, float w_ce, float w_dice,
                       void *stream);
int mvd_dcbce_bwd(const float *logits, const float *target, int target_form, const uint32_t *lut_host, const float *coef,
                  const float *loss, const float *gscale_dev, float gscale_host, float *dlogits, int N, long V, int R,
                  float w_ce, void *stream);
size_t mvd_dcce_masked_workspace_bytes(int N, long V, int K);
int mvd_dcce_masked_fwd(const float *logits, const float *target, float *stats, int N, long V, int K, int ignore_label,
                        void *ws, size_t ws_bytes, void *stream);
int mvd_dcce_masked_finalize(const float *stats, int N, const float *dstats, int Nd, float *loss, float *coef, long V, int K,
                             int batch_dice, int do_bg, float smooth, float w_ce, float w_dice, void *stream);
int mvd_dcce_masked_bwd(const float *logits, const float *target, const float *coef, const float *loss,
                        const float *gscale_dev, float gscale_host, float *dlogits, int N, long V, int K, float w_ce,
                        int ignore_label, void *stream);
int mvd_sigmoid_counts(const float *logits, const float *target, int target_form, const uint32_t *lut_host,
                       long long *counts, int N, long V, int R, void *stream);
int mvd_argmax_counts_masked(const float *logits, const float *target, long long *counts, int N, long V, int K,
                             int ignore_label, void *stream);
int mvd_seg_to_regions(const float *seg, const uint32_t *lut_host, float *planes, int N, long V, int R, int with_ignore,
                       void *stream);
/* ------------------------------------------------------------------------------------------------------------
 * Top-k cross entropy (csrc/loss_topk.hip): TopKLoss (robust_ce_loss.py:19-32) and the CE half of upstream
 * 2.1.1's DC_and_topk_loss, per deep-supervision level on planar fp32 logits [N,K,V], K <= 8, float label target [N,V].
 * Every stage is one or more plain launches on `stream`: nothing waits for another workgroup, nothing synchronises, all
 * state is in device memory -- capturable, and a replay repeats the eager step's bits (integer atomics, fixed-order sums).
 * ce_fwd: ce[n*V+v] = (1-eps)(-log p_t) + eps/K sum_j (-log p_j) >= +0.0 in fp32; +0.0 where the label is ignore_index
 *   (reduction='none': such voxels stay in the selection).
 * select: the exact k-th largest of the n = N*V values by a radix descent over their bit patterns (11 + 11 + 10 bits, a
 *   histogram launch and a one-workgroup scan launch per pass, after one launch that resets histograms and state).
 *   state (DEVICE uint32[4]) = {t_bits, cnt_gt, cnt_eq, rank within the ties}: the threshold's bit pattern, how many
 *   values lie strictly above it and how many equal it.  1 <= k <= n < 2^31; k == 0 is refused (the reference's mean
 *   over an empty selection is NaN).
 * finalize: loss[1] = (S_gt + (k - cnt_gt) t) / k with S_gt summed in fp64 in a fixed order, = torch.topk(ce, k).mean()
 *   whichever tied elements torch picks; loss[0] = w_ce * loss[1] + (dice_loss ? dice_loss[0] : 0), dice_loss = the
 *   loss[] of mvd_dcce_finalize / mvd_dcce_masked_finalize run with w_ce = 0.
 * bwd: dlogits[n,c,v] = g ( w_ce s/k (p_c - ((1-eps) y_c + eps/K)) + p_c (q_c - sum_j p_j q_j) ), q from coef as in
 *   mvd_dcce_bwd (coef may be NULL: no Dice term); s = 1 where ce > t, (k - cnt_gt)/cnt_eq where ce == t (ties share the
 *   remaining weight equally), 0 below; a voxel labelled ignore_index is an exact 0.  ce is the buffer ce_fwd wrote.
 * ws: mvd_topk_workspace_bytes, shared by select and finalize of one level (finalize does not touch the histograms). */
size_t mvd_topk_workspace_bytes(int N, long V);
int mvd_topk_ce_fwd(const float *logits, const float *target, float *ce, int N, long V, int K, int ignore_index,
                    float label_smoothing, void *stream);
int mvd_topk_select(const float *ce, long n, long k, uint32_t *state, void *ws, size_t ws_bytes, void *stream);
int mvd_topk_finalize(const float *ce, long n, long k, const uint32_t *state, float w_ce, const float *dice_loss, float *loss,
                      void *ws, size_t ws_bytes, void *stream);
int mvd_topk_bwd(const float *logits, const float *target, const float *ce, const uint32_t *state, const float *coef,
                 const float *gscale_dev, float gscale_host, float *dlogits, int N, long V, int K, long k, float w_ce,
                 int ignore_index, float label_smoothing, void *stream);
/* Region export (label_handling.py:163-171, :199-205), same tables / lerp order / walk as mvd_export_resize_argmax_u8:
 * mvd_export_resize_regions_u8: the label starts at 0; for i = 0..R-1 a voxel whose interpolated head i is > 0 (see
 *   mvd_sigmoid_counts for the rule) becomes class_order[i] (HOST int[R], 0..255): the last matching head wins.
 * mvd_export_resize_sigmoid_f32: out = float [K] planes, 1 / (1 + exp(-z)) in fp32; every plane is 0 outside the bbox. */
int mvd_export_resize_regions_u8(const float *logits, unsigned char *out, const int *idx0, const int *idx1,
                                 const float *weight, int R, int d, int h, int w, int D, int H, int W, const int *full,
                                 const int *lo, const int *perm, const int *class_order, void *stream);
int mvd_export_resize_sigmoid_f32(const float *logits, float *out, const int *idx0, const int *idx1, const float *weight,
                                  int K, int d, int h, int w, int D, int H, int W, const int *full, const int *lo,
                                  const int *perm, void *stream);

/* Model ensembling (nnunetv2/ensembling/ensemble.py:17-46, predict_from_raw_data.py:483-497).
 * mvd_export_ensemble_argmax_u8: the fused ensemble export for plain labels.  M members (1..8), K heads (2..8).  logits,
 *   idx0, idx1, weight: HOST arrays of M DEVICE pointers -- member m's logits [K, dims[3m], dims[3m+1], dims[3m+2]] (dims:
 *   HOST int[3 M]) and its own tables as mvd_export_resize_argmax_u8 takes them; (D, H, W), full, lo, perm: the one output
 *   geometry all members share.  Per output voxel, members ascending, in fp32: the K logits interpolated as the single
 *   export does, softmax as mvd_export_resize_softmax_f32 (max, expf(v - max), sum with k ascending, e / sum), acc_k += p_k;
 *   mean_k = acc_k / M (a division; none for M == 1); out = the argmax with a strict > (the first index wins an exact
 *   tie), 0 outside the bbox.  mean != NULL: also the float [K] mean planes of the same volume, channel 0 is 1 outside
 *   the bbox.  Bit-identical to mvd_export_resize_softmax_f32 per member followed by mvd_ensemble_mean_argmax.
 * mvd_ensemble_mean_argmax: probs = HOST array of M (1..8) DEVICE pointers to float [K, n] volumes (K 1..8):
 *   avg = p_0; avg += p_m (m ascending); avg /= M; seg = uint8 argmax (strict >), mean != NULL: float [K, n] avg.
 *   16-byte loads when n % 4 == 0 and every base is 16-byte aligned, scalar otherwise.
 * mvd_sw_normalize_add: sum = first ? acc / npred : sum + acc / npred; with last != 0 and M > 1 then sum *= fp32(1 / M),
 *   which is what torch's device `sum /= M` computes.  sum may be acc. */
int mvd_export_ensemble_argmax_u8(const float *const *logits, const int *const *idx0, const int *const *idx1,
                                  const float *const *weight, const int *dims, int M, int K, int D, int H, int W,
                                  const int *full, const int *lo, const int *perm, unsigned char *out, float *mean,
                                  void *stream);
int mvd_ensemble_mean_argmax(const float *const *probs, int M, int K, long n, unsigned char *seg, float *mean,
                             void *stream);
int mvd_sw_normalize_add(float *sum, const float *acc, const float *npred, int K, long V, int first, int last, int M,
                         void *stream);

/* The bottleneck fusion block of FinalNetv2 (csrc/attention.hip): fp32, no atomics (bit-identical run to run).
 * Dropout: `state` is a DEVICE long long[2] = {seed, t}.  Element e of site s is kept iff the 24-bit uniform (w >> 40) 2^-24
 *   >= p, w = word e & 3 of Philox4x64-10 with key (seed, s) and counter ((e >> 2) + 1, t, 0, 0) (numpy.random.Philox(key =
 *   (seed, s), counter = (0, t, 0, 0)).random_raw()[e]); kept values are scaled by 1 / (1 - p).  p == 0: no dropout, state
 *   is not read.  mvd_dropout_tick: t += 1 (one launch at the head of a training-mode forward; the backward of that step
 *   reads the same t).  mvd_dropout_mask: the keep mask (1 / 0 bytes) of n elements of (seed, t, site): for tests.
 * mvd_layernorm_fwd: rows [M, C]; pos != NULL: xs = x + pos[m % Npos] first (xs is written when non-NULL), y = (xs - mean)
 *   rstd gamma + beta with the variance as the mean of the centred squares (two passes), mean / rstd [M] saved.
 * mvd_layernorm_bwd: dx = LayerNorm'(dy) [+ dres1] [+ dres2]; dxd != NULL: also dxd = dx * (dropout factor of element
 *   m C + c of `site`): the input gradient of a linear whose epilogue dropped; dgamma, dbeta [C]; dpos != NULL:
 *   dpos[n] = sum over the batch of dx (M = batch x Npos, batch <= 64).  One launch.
 * mvd_linear_fwd: y[M, O] = (x[M, C] w[O, C]^T + bias) * (dropout factor of element m O + o) + res; bias, res optional.
 *   v_mfma_f32_16x16x4_f32 through bounds-checked loaders: M arbitrary, C and O multiples of 8.
 * mvd_linear_bwd: g = dy (already multiplied by the dropout factors): dx = g w (skipped when NULL), dw = g^T x,
 *   db = sum_m g (optional): one launch per gradient, db in dw's.
 * mvd_attention_fwd: H heads of dh over [B, N, 3 H dh] buffers (channel = which (H dh) + head dh + j): queries from qbuf,
 *   keys and values from kvbuf (the same buffer for self-attention), out[B, N, H dh] = dropout(softmax(q k^T dh^-1/2)) v
 *   [+ res]; the row maximum is subtracted; rowmax / rowsum [B H N] saved.  N <= 256, 4 <= dh <= 64, dh % 4 == 0.
 * mvd_attention_bwd: recomputes the probabilities from q, k, rowmax and rowsum; dq into dqbuf's q section, dk and dv into
 *   dkvbuf's k and v sections (same layout as the inputs); delta [B H N] is scratch.  Two launches. */
int mvd_dropout_tick(long long *state, void *stream);
int mvd_dropout_mask(unsigned long long seed, unsigned long long t, int site, float p, long n, unsigned char *out,
                     void *stream);
int mvd_layernorm_fwd(const float *x, const float *pos, float *xs, float *y, float *mean, float *rstd, const float *gamma,
                      const float *beta, long M, int C, long Npos, float eps, void *stream);
int mvd_layernorm_bwd(const float *dy, const float *xs, const float *mean, const float *rstd, const float *gamma,
                      const float *dres1, const float *dres2, float *dx, float *dxd, float *dgamma, float *dbeta,
                      float *dpos, long M, int C, long Npos, const long long *state, float p, int site, void *stream);
int mvd_linear_fwd(const float *x, const float *w, const float *bias, const float *res, float *y, long M, int C, int O,
                   const long long *state, float p, int site, void *stream);
int mvd_linear_bwd(const float *g, const float *x, const float *w, float *dx, float *dw, float *db, long M, int C, int O,
                   void *stream);
int mvd_attention_fwd(const float *qbuf, const float *kvbuf, const float *res, float *out, float *rowmax, float *rowsum, int B,
                      int N, int H, int dh, const long long *state, float p, int site, void *stream);
int mvd_attention_bwd(const float *qbuf, const float *kvbuf, const float *dout, const float *rowmax, const float *rowsum,
                      float *delta, float *dqbuf, float *dkvbuf, int B, int N, int H, int dh, const long long *state, float p,
                      int site, void *stream);

/* Level-set persistence, dimensions 0 and 1, of P = B * n_channels planes of a [B,C,H,W] tensor on the Freudenthal
 * triangulation (nn/levelset.py:64-93: vertices row-major, width = W; edges horizontal, vertical, one diagonal
 * (ind, ind+W+1) per square; the two triangles of each square), and the persistence topological loss on top of it
 * (loss/Topo_Loss.py:16-85).  Lower-star filtration of g = f or -f (-0 folded to +0), total order (value, dimension,
 * index within the dimension); the critical vertex of a cell is its first maximal vertex (complex.cpp:142).
 *   mvd_ls2d_num_cells: n = V + E (+ T for maxdim 1) cells per problem; V, E, T through the pointers (may be NULL).
 *   mvd_ls2d_sorted_keys (device): keys_sorted [P][n], ascending per problem, key = ord(value) << 32 | dimension << 30 |
 *       index; problem p = b * n_channels + j is plane (b, channels[j]).  One key kernel + one in-place merge sort per
 *       problem (no kernel of either waits on another workgroup).
 *   mvd_ls2d_pair_host (host, plain C++, <= 16 threads): bars [P][V+T][4] int32 = {bits of the birth value, bits of the
 *       death value, birth critical vertex, death critical vertex}: rows [0,V) the dimension-0 bars in vertex order (the
 *       essential bar dies at +inf, -inf for super-level, death vertex -1), rows [V,V+T) the dimension-1 bars in the
 *       order of their killing triangles; values carry the sign of the input.  edge_row [P][E]: the bar row each edge
 *       is an endpoint of (< V: death of a dimension-0 bar, >= V: birth of a dimension-1 bar; -1 with maxdim 0 for an edge
 *       that opens a cycle).
 *   mvd_ls2d_topk: lengths / index [P][2][k], the k longest bars per dimension, descending (end - start of
 *       get_start_end, infinite and NaN -> 0, zero padded; index = bar row, -1 for padding and zero-length bars), 1<=k<=64.
 *   mvd_ls2d_topk_bwd: g_bars [P][V+T][2] = d lengths scattered onto the (birth, death) entries, zero elsewhere.
 *   mvd_ls2d_topoloss_fwd: out[0] = (1/B) sum_{b,i,dim,j} s * lengths^2, s = -1 for j < label[b][idx[i]][dim] else +1
 *       (label int32 [B][n_label][2]); fp64, fixed order.   mvd_ls2d_topoloss_bwd: its gradient times g_out[0], written
 *       into grad [B][C][H][W] (class idx[i] is channel idx[i] + 1), every vertex summed in a fixed order.
 *   mvd_ls2d_diagram_bwd: persistence_backward (cohom.cpp:148-196) as a gather per vertex; g0 [P][V][2], g1 [P][T][2].
 *   mvd_ls2d_count_bars: counts [P][2] = bars of non-zero length per dimension (the essential bar iff born != 0).
 *   mvd_ls2d_onehot: planes [B][C][V] = (label [B][V] == c). */
long mvd_ls2d_num_cells(int H, int W, int maxdim, long *nv, long *ne, long *nt);
size_t mvd_ls2d_workspace_bytes(int P, int H, int W, int maxdim);
int mvd_ls2d_sorted_keys(const float *x, int B, int C, int H, int W, const int *channels, int n_channels, int sublevel,
                         int maxdim, uint64_t *keys_sorted, void *ws, size_t ws_bytes, void *stream);
int mvd_ls2d_pair_host(const uint64_t *keys_host, int P, int H, int W, int sublevel, int maxdim, int32_t *bars,
                       int32_t *edge_row, int n_threads);
int mvd_ls2d_topk(const int32_t *bars, int P, int H, int W, int maxdim, int sublevel, int k, float *lengths, int32_t *index,
                  void *stream);
int mvd_ls2d_topk_bwd(const float *g_lengths, const int32_t *index, int P, int H, int W, int maxdim, int sublevel, int k,
                      float *g_bars, void *stream);
int mvd_ls2d_topoloss_fwd(const float *lengths, const int32_t *label, int B, const int *idx, int n_idx, int n_label, int k,
                          float *out, void *stream);
int mvd_ls2d_topoloss_bwd(const float *lengths, const int32_t *index, const int32_t *bars, const int32_t *label,
                          const float *g_out, int B, int C, int H, int W, const int *idx, int n_idx, int n_label, int k,
                          int sublevel, float *grad, void *stream);
int mvd_ls2d_diagram_bwd(const float *g0, const float *g1, const int32_t *bars, const int32_t *edge_row, int B, int C, int H,
                         int W, const int *channels, int n_channels, int maxdim, float *grad, void *stream);
int mvd_ls2d_count_bars(const int32_t *bars, int P, int H, int W, int sublevel, int32_t *counts, void *stream);
int mvd_ls2d_onehot(const float *label, float *planes, int B, int C, long V, void *stream);

/* 3-D cubical persistence, dimensions 0 and 2, of N fields f [N,D,H,W] (sublevel filtration, voxels as closed
 * top-dimensional cells: gudhi's top_dimensional_cells, CubicalComplex(dim=3) of MVDTrainer.py:94-97), and the
 * q-Wasserstein loss (L-inf ground metric, the diagonal allowed) against the diagram of a binary mask, m copies of the
 * point (0, 1) (MVDTrainer.py:907-925, training/loss/TopoLoss.py).  Dimension 0 = elder-rule H0 of the 26-neighbourhood
 * graph with edge value max; dimension 2 = by Alexander duality the elder-rule H0 of the voxels in descending order on
 * the 6-neighbourhood with edge value min and one outside vertex of value +inf joined to every border voxel.  Dimension 1
 * needs a boundary-matrix reduction and is refused.  Ties: vertices by (value, linear index), edges by (value,
 * enumeration index), -0 folded to +0, as mvd_h0_*.  Essential bars are dropped.
 *   mvd_cub3d_num_keys: slots per sample (V * 13 or V * 4); *n_valid (may be NULL) of them are edges and sort first.
 *   mvd_cub3d_sorted_keys (device): keys_sorted [N][slots] ascending per sample, key = ord(value) << 32 | (v * n_off + k).
 *   mvd_cub3d_pair_host (host, plain C++, <= 16 threads): from f_host [N][V] and the first n_keys = n_valid sorted keys of
 *       every sample, bars [N][V][2] int32 = (birth voxel, death voxel) of the bars with death > birth in sweep order,
 *       counts [N] of them.  Dimension 0: birth = the dying component's minimum, death = the arg-max vertex of the
 *       merging edge; dimension 2: birth = the arg-min vertex of the merging edge, death = the dying component's maximum.
 *   mvd_cub3d_target_count (device): m [N] int32 -- dimension 2: 6-connected foreground components touching no face of
 *       the volume; dimension 0: 26-connected background components - 1, floored at 0.
 *   mvd_cub3d_match_fwd: per bar c0 = (d-b)/2, c1 = max(|b|, |1-d|), gain = c0^q + 2^-q - c1^q in fp64; selected = the
 *       <= m bars of largest strictly positive gain (ties to the lower bar index); wq [N] = W^q in fp64, fixed order;
 *       out[0] = mean_n wq[n]^(1/q).  bars [n_total][2] of all samples, sample n = rows [offsets[n], offsets[n+1]).
 *   mvd_cub3d_scatter_plan: the gradient entries (2 per bar) sorted by the voxel they land on (selected == NULL: all).
 *   mvd_cub3d_match_bwd: grad [N][V] zeroed, then one launch; one thread sums a voxel's run in a fixed order.
 *   mvd_cub3d_diagram_bwd: the same scatter of a diagram gradient g_diag [n_total][2]. */
long mvd_cub3d_num_keys(int D, int H, int W, int dim, long *n_valid);
size_t mvd_cub3d_workspace_bytes(int D, int H, int W, int dim);
int mvd_cub3d_sorted_keys(const float *f, int N, int D, int H, int W, int dim, uint64_t *keys_sorted, void *ws,
                          size_t ws_bytes, void *stream);
int mvd_cub3d_pair_host(const float *f_host, const uint64_t *keys_host, long n_keys, int N, int D, int H, int W, int dim,
                        int32_t *bars, int32_t *counts, int n_threads);
size_t mvd_cub3d_target_workspace_bytes(int D, int H, int W);
int mvd_cub3d_target_count(const float *target, int N, int D, int H, int W, int dim, int32_t *m, void *ws, size_t ws_bytes,
                           void *stream);
size_t mvd_cub3d_match_workspace_bytes(long n_total);
int mvd_cub3d_match_fwd(const float *field, const int32_t *bars, const int32_t *offsets_host, const int32_t *offsets_dev,
                        const int32_t *m, int N, long V, double q, uint8_t *selected, double *wq, float *out, void *ws,
                        size_t ws_bytes, void *stream);
int mvd_cub3d_scatter_plan(const float *field, const int32_t *bars, const int32_t *offsets_dev, const uint8_t *selected, int N,
                           long V, long n_total, uint32_t *key_sorted, uint32_t *order, void *ws, size_t ws_bytes,
                           void *stream);
int mvd_cub3d_match_bwd(const float *field, const int32_t *bars, const int32_t *offsets_dev, const uint8_t *selected,
                        const double *wq, const float *g_out, const uint32_t *key_sorted, const uint32_t *order, int N, long V,
                        long n_total, double q, float *grad, void *stream);
int mvd_cub3d_diagram_bwd(const float *g_diag, const uint32_t *key_sorted, const uint32_t *order, int N, long V, long n_total,
                          float *grad, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MVDSEG_HIP_H */
