// Top-k cross entropy: TopKLoss / DC_and_topk_loss of nnU-Net's loss trainer variants on planar fp32 logits
// [N][K][V] with a float label target [N][V].  Per voxel CE (optionally label-smoothed) -> exact k-th largest value by an
// MSB-first radix descent over the uint32 bit patterns (non-negative floats order as their bits) -> mean of the k largest.
// Structure: every stage is its own launch on the caller's stream; no kernel waits for another workgroup; all state (the
// histograms, the descent state) lives in device memory and is reset by a launch of its own, so the chain is capturable
// and a replay repeats the eager bits.  Integer atomics only (they commute: the result does not depend on arrival order);
// the one float sum is fp64 per thread -> fixed-order block tree -> partials -> one wave (the k_dcce_fwd convention).
#include "common.h"

namespace mvd {

constexpr int TKMAX = 8;        // classes (the KMAX of loss.hip)
constexpr int TK_BINS = 2048;   // bins of one pass's histogram (11 bits; the last pass uses 1024 of them)
constexpr int TK_PASSES = 3;    // bits 31..21, 20..10, 9..0
// state[4]: {t_bits (the prefix chosen so far during the descent), cnt_gt, cnt_eq, remaining rank}
enum { TS_BITS = 0, TS_GT = 1, TS_EQ = 2, TS_RANK = 3 };

__device__ __forceinline__ int tk_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__device__ __forceinline__ int tk_nbins(int pass) { return pass == 2 ? 1024 : 2048; }

// ce[n*V + v] = (1 - eps) * (-log p_y) + eps / K * sum_j (-log p_j), every term as log(sum exp(z - max)) - (z_j - max) >= 0;
// a voxel whose label is `ignore` stores +0.0 (cross_entropy(reduction='none'): it still takes part in the selection).
__global__ __launch_bounds__(256) void k_topk_ce_fwd(const float *__restrict__ logits, const float *__restrict__ target,
                                                     float *__restrict__ ce, long V, int K, int ignore, float eps) {
    const int n = blockIdx.y;
    const float *ln = logits + (size_t)n * K * V;
    const float *tn = target + (size_t)n * V;
    float *cn = ce + (size_t)n * V;
    const float epsk = eps / (float)K;
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        float z[TKMAX];
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < TKMAX; k++) z[k] = ln[(size_t)(k < K ? k : K - 1) * V + v];  // all classes in flight (no predicate)
#pragma unroll
        for (int k = 0; k < TKMAX; k++)
            if (k < K) m = fmaxf(m, z[k]);
        const int yi = (int)tn[v];  // .long() truncation
        const int y = yi < 0 ? 0 : (yi >= K ? K - 1 : yi);
        float s = 0.f, zy = 0.f, zs = 0.f;
#pragma unroll
        for (int k = 0; k < TKMAX; k++)
            if (k < K) {
                const float d = z[k] - m;
                if (k == y) zy = d;
                zs += d;
                s += expf(d);
            }
        const float lse = logf(s);  // s >= 1: lse >= 0, and every d <= 0
        const float c = (1.f - eps) * (lse - zy) + epsk * ((float)K * lse - zs);
        cn[v] = yi == ignore ? 0.f : fmaxf(c, 0.f);  // (fmaxf: no -0.0, whose bit pattern would sort above everything)
    }
}

__global__ void k_topk_reset(uint32_t *__restrict__ hist, uint32_t *__restrict__ state, uint32_t k) {
    for (int i = threadIdx.x; i < TK_PASSES * TK_BINS; i += blockDim.x) hist[i] = 0u;
    if (threadIdx.x == 0) {
        state[TS_BITS] = 0u;
        state[TS_GT] = 0u;
        state[TS_EQ] = 0u;
        state[TS_RANK] = k;
    }
}

// Histogram of the pass's digit over the values whose higher bits equal the prefix chosen so far.  LDS histogram per
// workgroup, flushed with one integer atomic per occupied bin.  Many voxels share the leading bits of their CE (all of
// them in the worst case), and 64 LDS atomics of one wave on one address run one after the other: the lanes that hold
// the digit of the wave's first live lane are counted by ONE atomic (ballot + popcount), twice over, and only what is left
// after two such rounds goes to the LDS one lane at a time.  (Measured, DESIGN 29: within 4 % of plain LDS atomics either
// way on the MI355X, all-equal input included -- kept as the guard for that case, not as a speed-up.)
__global__ __launch_bounds__(256) void k_topk_hist(const float *__restrict__ ce, long n, const uint32_t *__restrict__ state,
                                                   uint32_t *__restrict__ hist, int pass) {
    __shared__ uint32_t h[TK_BINS];
    const int nb = tk_nbins(pass), sh = tk_shift(pass);
    for (int i = threadIdx.x; i < nb; i += 256) h[i] = 0u;
    __syncthreads();
    const uint32_t prefix = state[TS_BITS];
    const int hs = pass == 0 ? 32 : (pass == 1 ? 21 : 10);   // bits above this position are the prefix
    const int lane = threadIdx.x & 63;
    // wave-uniform trip count: every lane of a wave takes part in the ballots
    for (long base = (long)blockIdx.x * 256; base < n; base += (long)gridDim.x * 256) {
        const long i = base + threadIdx.x;
        uint32_t bits = 0u;
        bool live = i < n;
        if (live) bits = __float_as_uint(ce[i]);
        if (pass > 0) live = live && ((bits >> hs) == (prefix >> hs));
        const uint32_t d = (bits >> sh) & (uint32_t)(nb - 1);
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const unsigned long long rest = __ballot(live);
            if (rest == 0ull) break;
            const uint32_t lead = (uint32_t)__shfl((int)d, __ffsll((long long)rest) - 1, 64);
            const unsigned long long same = __ballot(live && d == lead);
            if (lane == __ffsll((long long)same) - 1) atomicAdd(&h[lead], (uint32_t)__popcll(same));
            live = live && d != lead;
        }
        if (live) atomicAdd(&h[d], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&hist[i], c);
    }
}

// One workgroup: walk the pass's bins from the top, find the bin that holds the element of rank state[TS_RANK] (1-based,
// counted from the largest), append its digit to the prefix, add what lies above it to cnt_gt and take it off the rank.
// After the last pass the prefix is the threshold's bit pattern and the bin's count is cnt_eq.
__global__ __launch_bounds__(256) void k_topk_scan(const uint32_t *__restrict__ hist, uint32_t *__restrict__ state, int pass) {
    __shared__ uint32_t part[256];
    const int nb = tk_nbins(pass), sh = tk_shift(pass);
    const int per = nb / 256;  // 8 or 4 consecutive bins per thread, thread 0 holds the top ones
    const int t = threadIdx.x;
    const int top = nb - 1 - t * per;
    const uint32_t rank = state[TS_RANK];  // (read by every thread in front of the barriers, rewritten behind them)
    uint32_t c[8];
    uint32_t s = 0u;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        c[j] = j < per ? hist[top - j] : 0u;
        s += c[j];
    }
    part[t] = s;
    __syncthreads();
    if (t == 0) {  // exclusive sums from the top, 256 terms
        uint32_t run = 0u;
        for (int i = 0; i < 256; i++) {
            const uint32_t x = part[i];
            part[i] = run;
            run += x;
        }
    }
    __syncthreads();
    uint32_t above = part[t];
    if (rank > above && rank <= above + s) {  // exactly one thread (1 <= rank <= the pass's total)
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (j < per) {
                if (rank > above && rank <= above + c[j]) {
                    state[TS_BITS] = state[TS_BITS] | ((uint32_t)(top - j) << sh);
                    state[TS_GT] = state[TS_GT] + above;
                    state[TS_RANK] = rank - above;
                    if (pass == TK_PASSES - 1) state[TS_EQ] = c[j];
                }
                above += c[j];
            }
    }
}

// partial[b] = sum of the values strictly above the threshold (fp64, fixed order)
__global__ __launch_bounds__(256) void k_topk_sum(const float *__restrict__ ce, long n, const uint32_t *__restrict__ state,
                                                  double *__restrict__ partial) {
    __shared__ double red[16];
    const uint32_t tb = state[TS_BITS];
    double acc[1] = {0.0};
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float c = ce[i];
        if (__float_as_uint(c) > tb) acc[0] += (double)c;
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}

// loss[1] = (S_gt + (k - cnt_gt) * t) / k (= torch.topk(ce, k).mean() whichever tied elements torch picks);
// loss[0] = w_ce * loss[1] + (dice ? dice[0] : 0) -- dice[0] is loss[0] of mvd_dcce_finalize run with w_ce = 0
__global__ void k_topk_finish(const double *__restrict__ partial, int nblk, const uint32_t *__restrict__ state, uint32_t k,
                              float w_ce, const float *__restrict__ dice, float *__restrict__ loss) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) s += partial[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) {
        const double t = (double)__uint_as_float(state[TS_BITS]);
        const float topk = (float)((s + (double)(k - state[TS_GT]) * t) / (double)k);
        loss[1] = topk;
        loss[0] = w_ce * topk + (dice ? dice[0] : 0.f);
    }
}

// dlogits[n,c,v] = g * ( w_ce * s / k * (p_c - ((1 - eps) y_c + eps / K)) + p_c * (q_c - sum_j p_j q_j) ),
// s = 1 above the threshold, (k - cnt_gt) / cnt_eq on it, 0 below; an ignored voxel is an exact 0 (its Dice term too: the
// Dice of DC_and_topk_loss is masked by the same label).  ce is the buffer the forward wrote: forward and backward
// cannot disagree about a voxel near the threshold.  q as in k_dcce_bwd (coef may be null: no Dice term).
__global__ __launch_bounds__(256) void k_topk_bwd(const float *__restrict__ logits, const float *__restrict__ target,
                                                  const float *__restrict__ ce, const uint32_t *__restrict__ state,
                                                  const float *__restrict__ coef, const float *__restrict__ gscale_dev,
                                                  float gscale_host, float *__restrict__ dlogits, long V, int K, uint32_t k,
                                                  float w_ce, int ignore, float eps) {
    const int n = blockIdx.y;
    const float *ln = logits + (size_t)n * K * V;
    const float *tn = target + (size_t)n * V;
    const float *cn = ce + (size_t)n * V;
    float *dn = dlogits + (size_t)n * K * V;
    const float g = gscale_host * (gscale_dev ? gscale_dev[0] : 1.0f);
    const uint32_t tb = state[TS_BITS];
    const float cew = w_ce / (float)k;
    const float share = cew * ((float)(k - state[TS_GT]) / (float)state[TS_EQ]);  // (cnt_eq >= 1: the k-th element itself)
    const float epsk = eps / (float)K, on = (1.f - eps) + epsk;
    float cI[TKMAX], cP[TKMAX];
#pragma unroll
    for (int c = 0; c < TKMAX; c++) {
        cI[c] = (coef && c < K) ? coef[((size_t)n * K + c) * 2 + 0] : 0.f;
        cP[c] = (coef && c < K) ? coef[((size_t)n * K + c) * 2 + 1] : 0.f;
    }
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
        float z[TKMAX];
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < TKMAX; c++) z[c] = ln[(size_t)(c < K ? c : K - 1) * V + v];  // all classes in flight (no predicate)
        const uint32_t cb = __float_as_uint(cn[v]);
#pragma unroll
        for (int c = 0; c < TKMAX; c++)
            if (c < K) m = fmaxf(m, z[c]);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < TKMAX; c++)
            if (c < K) {
                z[c] = expf(z[c] - m);
                s += z[c];
            }
        const float inv = 1.0f / s;
        const int yi = (int)tn[v];
        const bool valid = yi != ignore;
        const int y = yi < 0 ? 0 : (yi >= K ? K - 1 : yi);
        const float wv = cb > tb ? cew : (cb == tb ? share : 0.f);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < TKMAX; c++)
            if (c < K) {
                z[c] *= inv;  // p_c
                const float q = cP[c] + (c == y ? cI[c] : 0.f);
                dot += z[c] * q;
            }
#pragma unroll
        for (int c = 0; c < TKMAX; c++)
            if (c < K) {
                const float q = cP[c] + (c == y ? cI[c] : 0.f);
                const float d = wv * (z[c] - (c == y ? on : epsk)) + z[c] * (q - dot);
                dn[(size_t)c * V + v] = valid ? g * d : 0.f;  // (a select, not a product: an exact 0)
            }
    }
}

}  // namespace mvd

using namespace mvd;

static inline long tgrid_for(long n, long cap) {
    long b = cdiv(n, 256);
    if (b > cap) b = cap;
    return b < 1 ? 1 : b;
}
static inline long tcap_per_n(long total_blocks, int N) {
    const long c = total_blocks / (N > 0 ? N : 1);
    return c > 0 ? c : 1;
}
// block caps of the wrappers (the grid-stride loops take the rest): DESIGN 29 lists the shapes that cross them
constexpr long TK_CAP_FWD = 2048, TK_CAP_HIST = 2048, TK_CAP_SUM = 1024, TK_CAP_BWD = 4096;

static inline bool topk_shape_ok(int N, long V, int K) {
    return N > 0 && N <= 65535 && V > 0 && K >= 2 && K <= TKMAX && (long)N * V < (1L << 31);
}

extern "C" {

// [hist: 3 x 2048 uint32][partial sums: <= 1024 double]
size_t mvd_topk_workspace_bytes(int N, long V) {
    (void)N;
    (void)V;
    return (size_t)TK_PASSES * TK_BINS * sizeof(uint32_t) + (size_t)TK_CAP_SUM * sizeof(double) + 256;
}

int mvd_topk_ce_fwd(const float *logits, const float *target, float *ce, int N, long V, int K, int ignore_index,
                    float label_smoothing, void *stream) {
    MVD_REQUIRE(logits && target && ce, "topk_ce_fwd: null pointer");
    MVD_REQUIRE(topk_shape_ok(N, V, K), "topk_ce_fwd: bad shape (2 <= K <= 8 classes, fewer than 2^31 voxels)");
    MVD_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, "topk_ce_fwd: label_smoothing must lie in [0, 1]");
    const long bx = tgrid_for(V, tcap_per_n(TK_CAP_FWD, N));
    hipLaunchKernelGGL(k_topk_ce_fwd, dim3(bx, N), dim3(256), 0, as_stream(stream), logits, target, ce, V, K, ignore_index,
                       label_smoothing);
    return check_launch("topk_ce_fwd");
}

int mvd_topk_select(const float *ce, long n, long k, uint32_t *state, void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(ce && state && ws, "topk_select: null pointer");
    MVD_REQUIRE(n > 0 && n < (1L << 31), "topk_select: 1 <= n < 2^31 values");
    MVD_REQUIRE(k >= 1 && k <= n, "topk_select: k = %ld of n = %ld values (k == 0: fewer than 100 / k_percent voxels; the "
                "reference's mean over an empty selection is NaN)", k, n);
    MVD_REQUIRE(ws_bytes >= mvd_topk_workspace_bytes(1, n), "topk_select: workspace too small");
    hipStream_t s = as_stream(stream);
    uint32_t *hist = reinterpret_cast<uint32_t *>(ws);
    hipLaunchKernelGGL(k_topk_reset, dim3(1), dim3(256), 0, s, hist, state, (uint32_t)k);
    if (check_launch("topk_select (reset)")) return 1;
    const long bx = tgrid_for(n, TK_CAP_HIST);
    for (int pass = 0; pass < TK_PASSES; pass++) {
        hipLaunchKernelGGL(k_topk_hist, dim3(bx), dim3(256), 0, s, ce, n, state, hist + (size_t)pass * TK_BINS, pass);
        if (check_launch("topk_select (histogram)")) return 1;
        hipLaunchKernelGGL(k_topk_scan, dim3(1), dim3(256), 0, s, hist + (size_t)pass * TK_BINS, state, pass);
        if (check_launch("topk_select (scan)")) return 1;
    }
    return 0;
}

int mvd_topk_finalize(const float *ce, long n, long k, const uint32_t *state, float w_ce, const float *dice_loss, float *loss,
                      void *ws, size_t ws_bytes, void *stream) {
    MVD_REQUIRE(ce && state && loss && ws, "topk_finalize: null pointer");
    MVD_REQUIRE(n > 0 && n < (1L << 31) && k >= 1 && k <= n, "topk_finalize: bad n / k");
    MVD_REQUIRE(ws_bytes >= mvd_topk_workspace_bytes(1, n), "topk_finalize: workspace too small");
    hipStream_t s = as_stream(stream);
    double *partial = reinterpret_cast<double *>(reinterpret_cast<char *>(ws) + (size_t)TK_PASSES * TK_BINS * sizeof(uint32_t));
    const long bx = tgrid_for(n, TK_CAP_SUM);
    hipLaunchKernelGGL(k_topk_sum, dim3(bx), dim3(256), 0, s, ce, n, state, partial);
    if (check_launch("topk_finalize (sum)")) return 1;
    hipLaunchKernelGGL(k_topk_finish, dim3(1), dim3(64), 0, s, partial, (int)bx, state, (uint32_t)k, w_ce, dice_loss, loss);
    return check_launch("topk_finalize");
}

int mvd_topk_bwd(const float *logits, const float *target, const float *ce, const uint32_t *state, const float *coef,
                 const float *gscale_dev, float gscale_host, float *dlogits, int N, long V, int K, long k, float w_ce,
                 int ignore_index, float label_smoothing, void *stream) {
    MVD_REQUIRE(logits && target && ce && state && dlogits, "topk_bwd: null pointer");
    MVD_REQUIRE(topk_shape_ok(N, V, K), "topk_bwd: bad shape (2 <= K <= 8 classes, fewer than 2^31 voxels)");
    MVD_REQUIRE(k >= 1 && k <= (long)N * V, "topk_bwd: bad k");
    const long bx = tgrid_for(V, tcap_per_n(TK_CAP_BWD, N));
    hipLaunchKernelGGL(k_topk_bwd, dim3(bx, N), dim3(256), 0, as_stream(stream), logits, target, ce, state, coef, gscale_dev,
                       gscale_host, dlogits, V, K, (uint32_t)k, w_ce, ignore_index, label_smoothing);
    return check_launch("topk_bwd");
}
}
