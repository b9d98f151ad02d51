// Cascade stage of the on-device training feed: the transforms nnU-Net adds for 3d_cascade_fullres
// (nnUNetTrainer.py:740-755, custom_transforms/cascade_transforms.py) on the one-hot channels of the previous stage's
// segmentation.
//   MoveSegAsOneHotToData           k_cas_onehot: seg channel 1 -> K planes of 0/1 floats behind the modalities
//   ApplyRandomBinaryOperator       k_cas_pack / k_cas_morph / k_cas_apply / k_cas_unpack: ball dilation, erosion,
//                                   closing, opening on 64-bit bit-planes, then the added-voxel rule on the other planes
//   RemoveRandomConnectedComponent  k_cas_mask, mvd_cc_label(26), mvd_cc_component_sizes, k_cas_count / k_cas_pick /
//                                   k_cas_clear: remove valid component number floor(u n_valid) in label order
// Integer and bit work only, plain launches, no float atomics, no kernel waits on another; every parameter is a host
// value copied into the kernel arguments, so each call is capturable.  Bit-exact against scipy.ndimage.
//
// Bit-plane layout: plane [D][H][Wq] of 64-bit words, Wq = ceil(W / 64); bit b of word q is voxel x = 64 q + b.  The pad
// bits of the last word are 0 in every stored plane.
//
// Morphology.  The host gives the structuring element per (dz, dy) row as one x-interval [lo, hi] of READ offsets of the
// erosion, o = index - n / 2 (scipy centres an even-sided element at n / 2): erosion is out[p] = AND_o in[p + o], the
// dilation reads the negated offsets, out[p] = OR_o in[p - o].  Outside the volume counts as 0 for the dilation and as
// 1 for the erosion (border_value=True), pad bits included.  Both are computed as an OR: the erosion stages the
// COMPLEMENT of its input (outside -> 0 in both cases) and complements the result.  A workgroup of 256 threads makes a
// tile of 8 x 16 rows x 2 words; it stages the tile plus its (z, y) halo of the element's extent and one word either
// side in LDS (at most 24 x 32 x 4 words = 24 KiB), so each input word comes from HBM once per tile, not once per table
// row.  Per table row a thread reads (previous, current, next) word -- offsets are at most 8 bits -- into a 128-bit
// window, spreads the interval of length L by shift-doubling in ceil(log2 L) steps and takes the word at offset lo.
// LDS rows are 32 B apart, so the ds_read_b64 of 16 y-neighbours is 2-way bank-conflicted; the kernel is bound by the
// ~30 VALU operations per row, not by these reads.
//
// The reference skips an empty channel (`if not np.any(workon): continue`).  All four operators map an empty plane to an
// empty plane: a dilation of nothing is nothing, and the ball holds its centre offset for every r >= 1, so an erosion
// never sets a voxel that was clear.  Nothing is added either, so the device runs the operator unconditionally and needs
// no read-back for that rule.  The same holds for the removal: an empty channel has no valid root, and n_valid == 0
// makes the step a no-op.
#include "common.h"

namespace mvd {

typedef unsigned long long u64;

constexpr int CAS_MAX_ROWS = 256;  // 16 x 16 rows of a ball with r < 8
constexpr int CAS_TZ = 8, CAS_TY = 16, CAS_TXW = 2, CAS_HALO = 8;
constexpr int CAS_SXW = CAS_TXW + 2;

struct CasLabels {
    int n;
    float v[8];
};

struct CasTable {
    int n, hz, hy, erode;
    signed char dz[CAS_MAX_ROWS], dy[CAS_MAX_ROWS], lo[CAS_MAX_ROWS], hi[CAS_MAX_ROWS];
};

__global__ void k_cas_onehot(const float *__restrict__ seg, float *__restrict__ out, long n, CasLabels ls) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float s = seg[i];
        for (int k = 0; k < ls.n; k++) out[(size_t)k * n + i] = (s == ls.v[k]) ? 1.f : 0.f;
    }
}

// one wave per word: lane l reads voxel 64 q + l, the ballot is the word
__global__ void __launch_bounds__(256) k_cas_pack(const float *__restrict__ planes, u64 *__restrict__ bits, long rows,
                                                  int W, int Wq) {
    const int lane = threadIdx.x & 63;
    const long nwords = rows * Wq;
    for (long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6); w < nwords; w += (long)gridDim.x * 4) {
        const long row = w / Wq;
        const int x = (int)(w % Wq) * 64 + lane;
        const bool on = x < W && planes[row * W + x] != 0.f;
        const u64 word = __ballot(on);
        if (lane == 0) bits[w] = word;
    }
}

__global__ void k_cas_unpack(const u64 *__restrict__ bits, float *__restrict__ planes, long rows, int W, int Wq) {
    const long total = rows * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / W;
        const int x = (int)(i % W);
        planes[i] = ((bits[row * Wq + (x >> 6)] >> (x & 63)) & 1ull) ? 1.f : 0.f;
    }
}

__global__ void __launch_bounds__(256) k_cas_morph(const u64 *__restrict__ in, u64 *__restrict__ out, int D, int H, int W,
                                                   int Wq, CasTable t) {
    __shared__ u64 lds[(CAS_TZ + 2 * CAS_HALO) * (CAS_TY + 2 * CAS_HALO) * CAS_SXW];
    const int SZ = CAS_TZ + 2 * t.hz, SY = CAS_TY + 2 * t.hy;
    const int z0 = (int)blockIdx.z * CAS_TZ, y0 = (int)blockIdx.y * CAS_TY, q0 = (int)blockIdx.x * CAS_TXW;
    const u64 last_mask = (W & 63) ? ((1ull << (W & 63)) - 1ull) : ~0ull;
    for (int i = threadIdx.x; i < SZ * SY * CAS_SXW; i += 256) {
        const int sx = i % CAS_SXW, sy = (i / CAS_SXW) % SY, sz = i / (CAS_SXW * SY);
        const int gz = z0 - t.hz + sz, gy = y0 - t.hy + sy, gq = q0 - 1 + sx;
        u64 v = 0ull;
        if (gz >= 0 && gz < D && gy >= 0 && gy < H && gq >= 0 && gq < Wq) {
            v = in[((size_t)gz * H + gy) * Wq + gq];
            if (t.erode) v = ~v;
            if (gq == Wq - 1) v &= last_mask;
        }
        lds[i] = v;
    }
    __syncthreads();
    const int tx = threadIdx.x & 1, ty = (threadIdx.x >> 1) & 15, tz = threadIdx.x >> 5;
    u64 acc = 0ull;
    for (int r = 0; r < t.n; r++) {
        const int base = ((tz + t.hz + t.dz[r]) * SY + ty + t.hy + t.dy[r]) * CAS_SXW + tx + 1;
        const u64 P = lds[base - 1], R = lds[base], N = lds[base + 1];
        // window bit j holds voxel 64 q - 32 + j
        u64 wl = (P >> 32) | (R << 32), wh = (R >> 32) | (N << 32);
        const int L = t.hi[r] - t.lo[r] + 1;
        int cover = 1;
        while (cover < L) {  // T_c[j] = OR of window bits j .. j + c - 1
            const int m = (2 * cover <= L) ? cover : L - cover;
            const u64 sl = (wl >> m) | (wh << (64 - m)), sh = wh >> m;
            wl |= sl;
            wh |= sh;
            cover += m;
        }
        const int s = t.lo[r] + 32;  // 24 .. 40
        acc |= (wl >> s) | (wh << (64 - s));
    }
    const int gz = z0 + tz, gy = y0 + ty, gq = q0 + tx;
    if (gz < D && gy < H && gq < Wq) {
        if (t.erode) acc = ~acc;
        if (gq == Wq - 1) acc &= last_mask;
        out[((size_t)gz * H + gy) * Wq + gq] = acc;
    }
}

// planes[c] <- res; every other plane loses the voxels the operator added (cascade_transforms.py:128-134)
__global__ void k_cas_apply(u64 *__restrict__ planes, const u64 *__restrict__ res, int K, int c, long nwords) {
    for (long w = (long)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += (long)gridDim.x * blockDim.x) {
        const u64 r = res[w];
        const u64 keep = ~(r & ~planes[(size_t)c * nwords + w]);
        for (int k = 0; k < K; k++) {
            if (k == c) planes[(size_t)k * nwords + w] = r;
            else planes[(size_t)k * nwords + w] &= keep;
        }
    }
}

// ---------------------------------------------------------------------------------------------- component removal
__global__ void k_cas_mask(const float *__restrict__ chan, uint8_t *__restrict__ mask, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        mask[i] = chan[i] != 0.f;
}

// sizes[i] > 0 only at a component's root (its smallest linear index); a root is valid when its size is < thr.
// Block b counts the valid roots of its chunk [b chunk, (b + 1) chunk): integer sums, the same in any order.
__global__ void __launch_bounds__(256) k_cas_count(const int32_t *__restrict__ sizes, long n, long chunk, int32_t thr,
                                                   int32_t *__restrict__ blockcnt) {
    __shared__ int part[256];
    const long a = (long)blockIdx.x * chunk, b = a + chunk < n ? a + chunk : n;
    int cnt = 0;
    for (long i = a + threadIdx.x; i < b; i += 256) {
        const int32_t s = sizes[i];
        cnt += (s > 0 && s < thr);
    }
    part[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = part[0];
}

// chosen[0] = label (root + 1) of valid root number floor(u n_valid) in index order, 0 when there is none;
// chosen[1] = n_valid.  One workgroup; every step is a fixed-order scan.
__global__ void __launch_bounds__(256) k_cas_pick(const int32_t *__restrict__ sizes, long n, long chunk, int32_t thr,
                                                  const int32_t *__restrict__ blockcnt, int nblocks, double u,
                                                  int32_t *__restrict__ chosen) {
    __shared__ int part[256];
    __shared__ long sh_block, sh_rank;
    if (threadIdx.x == 0) {
        long total = 0;
        for (int b = 0; b < nblocks; b++) total += blockcnt[b];
        long blk = -1, rank = 0;
        if (total > 0) {
            long pick = (long)(u * (double)total);
            if (pick > total - 1) pick = total - 1;
            if (pick < 0) pick = 0;
            long before = 0;
            for (int b = 0; b < nblocks; b++) {
                const long c = blockcnt[b];
                if (pick < before + c) {
                    blk = b;
                    rank = pick - before;
                    break;
                }
                before += c;
            }
        }
        sh_block = blk;
        sh_rank = rank;
        chosen[1] = (int32_t)total;
        if (blk < 0) chosen[0] = 0;
    }
    __syncthreads();
    if (sh_block < 0) return;
    const long a = sh_block * chunk, b = a + chunk < n ? a + chunk : n;
    const long sub = (b - a + 255) / 256;
    const long ta = a + (long)threadIdx.x * sub, tb = ta + sub < b ? ta + sub : b;
    int cnt = 0;
    for (long i = ta; i < tb; i++) {
        const int32_t s = sizes[i];
        cnt += (s > 0 && s < thr);
    }
    part[threadIdx.x] = cnt;
    __syncthreads();
    long before = 0;
    for (int k = 0; k < (int)threadIdx.x; k++) before += part[k];
    const long rank = sh_rank - before;
    if (rank >= 0 && rank < cnt) {  // exactly one thread
        long seen = 0;
        for (long i = ta; i < tb; i++) {
            const int32_t s = sizes[i];
            if (s > 0 && s < thr) {
                if (seen == rank) {
                    chosen[0] = (int32_t)(i + 1);
                    break;
                }
                seen++;
            }
        }
    }
}

__global__ void k_cas_clear(const int32_t *__restrict__ labels, float *__restrict__ chan, float *__restrict__ other,
                            long n, const int32_t *__restrict__ chosen) {
    const int32_t l = chosen[0];
    if (l <= 0) return;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        if (labels[i] == l) {
            chan[i] = 0.f;
            if (other) other[i] = 1.f;
        }
    }
}

}  // namespace mvd

using namespace mvd;

static inline unsigned cas_grid(long n) {
    long b = cdiv(n, 256);
    if (b > 16384) b = 16384;
    return (unsigned)(b < 1 ? 1 : b);
}

static inline size_t cas_align(size_t v) { return (v + 255) & ~(size_t)255; }

static inline bool cas_shape_ok(int D, int H, int W) {
    return D > 0 && H > 0 && W > 0 && (long)D * H * W < 2147483647L && cdiv(D, CAS_TZ) <= 65535 && cdiv(H, CAS_TY) <= 65535;
}

static inline int cas_blocks(long n) {
    long b = cdiv(n, 1024);
    return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

static void cas_morph_launch(const u64 *in, u64 *out, int D, int H, int W, int Wq, const CasTable &t, hipStream_t s) {
    dim3 grid((unsigned)cdiv(Wq, CAS_TXW), (unsigned)cdiv(H, CAS_TY), (unsigned)cdiv(D, CAS_TZ));
    hipLaunchKernelGGL(k_cas_morph, grid, dim3(256), 0, s, in, out, D, H, W, Wq, t);
}

extern "C" {

int mvd_feed_cascade_onehot(const float *seg, float *out, long n, const int *labels, int K, void *stream) {
    MVD_REQUIRE(seg && out && labels, "feed_cascade_onehot: null pointer");
    MVD_REQUIRE(n > 0 && K >= 1 && K <= 8, "feed_cascade_onehot: 1..8 labels");
    CasLabels ls;
    ls.n = K;
    for (int i = 0; i < 8; i++) ls.v[i] = i < K ? (float)labels[i] : 0.f;
    hipLaunchKernelGGL(k_cas_onehot, dim3(cas_grid(n)), dim3(256), 0, as_stream(stream), seg, out, n, ls);
    return check_launch("feed_cascade_onehot");
}

size_t mvd_feed_cascade_plane_words(int D, int H, int W) {
    if (D <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)D * H * (size_t)cdiv(W, 64);
}

int mvd_feed_cascade_pack(const float *planes, uint64_t *bits, int K, int D, int H, int W, void *stream) {
    MVD_REQUIRE(planes && bits, "feed_cascade_pack: null pointer");
    MVD_REQUIRE(K >= 1 && K <= 8 && cas_shape_ok(D, H, W), "feed_cascade_pack: bad shape");
    const long rows = (long)K * D * H, Wq = cdiv(W, 64);
    long blocks = cdiv(rows * Wq, 4);
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_cas_pack, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), planes, (u64 *)bits, rows, W,
                       (int)Wq);
    return check_launch("feed_cascade_pack");
}

int mvd_feed_cascade_unpack(const uint64_t *bits, float *planes, int K, int D, int H, int W, void *stream) {
    MVD_REQUIRE(planes && bits, "feed_cascade_unpack: null pointer");
    MVD_REQUIRE(K >= 1 && K <= 8 && cas_shape_ok(D, H, W), "feed_cascade_unpack: bad shape");
    const long rows = (long)K * D * H;
    hipLaunchKernelGGL(k_cas_unpack, dim3(cas_grid(rows * W)), dim3(256), 0, as_stream(stream), (const u64 *)bits, planes,
                       rows, W, (int)cdiv(W, 64));
    return check_launch("feed_cascade_unpack");
}

int mvd_feed_cascade_morph(uint64_t *planes, uint64_t *tmp, int K, int c, int op, int D, int H, int W, const int *rows,
                           int nrows, void *stream) {
    MVD_REQUIRE(planes && tmp && rows, "feed_cascade_morph: null pointer");
    MVD_REQUIRE(K >= 1 && K <= 8 && c >= 0 && c < K && cas_shape_ok(D, H, W), "feed_cascade_morph: bad shape");
    MVD_REQUIRE(op >= 0 && op < 4, "feed_cascade_morph: op is 0 dilation, 1 erosion, 2 closing, 3 opening");
    MVD_REQUIRE(nrows >= 1 && nrows <= CAS_MAX_ROWS, "feed_cascade_morph: 1..256 table rows");
    CasTable ero, dil;
    memset(&ero, 0, sizeof(ero));
    ero.n = nrows;
    ero.erode = 1;
    for (int r = 0; r < nrows; r++) {
        const int dz = rows[4 * r], dy = rows[4 * r + 1], lo = rows[4 * r + 2], hi = rows[4 * r + 3];
        MVD_REQUIRE(dz >= -CAS_HALO && dz <= CAS_HALO && dy >= -CAS_HALO && dy <= CAS_HALO && lo >= -8 && lo <= hi && hi <= 8,
                    "feed_cascade_morph: table row %d out of range (offsets within +-8, lo <= hi)", r);
        ero.dz[r] = (signed char)dz;
        ero.dy[r] = (signed char)dy;
        ero.lo[r] = (signed char)lo;
        ero.hi[r] = (signed char)hi;
        const int az = dz < 0 ? -dz : dz, ay = dy < 0 ? -dy : dy;
        if (az > ero.hz) ero.hz = az;
        if (ay > ero.hy) ero.hy = ay;
    }
    dil = ero;
    dil.erode = 0;
    for (int r = 0; r < nrows; r++) {  // the dilation reads the negated offsets
        dil.dz[r] = (signed char)-ero.dz[r];
        dil.dy[r] = (signed char)-ero.dy[r];
        dil.lo[r] = (signed char)-ero.hi[r];
        dil.hi[r] = (signed char)-ero.lo[r];
    }
    hipStream_t s = as_stream(stream);
    const int Wq = (int)cdiv(W, 64);
    const long nwords = (long)D * H * Wq;
    u64 *src = (u64 *)planes + (size_t)c * nwords, *res = (u64 *)tmp, *mid = (u64 *)tmp + nwords;
    switch (op) {
        case 0: cas_morph_launch(src, res, D, H, W, Wq, dil, s); break;
        case 1: cas_morph_launch(src, res, D, H, W, Wq, ero, s); break;
        case 2:
            cas_morph_launch(src, mid, D, H, W, Wq, dil, s);
            cas_morph_launch(mid, res, D, H, W, Wq, ero, s);
            break;
        default:
            cas_morph_launch(src, mid, D, H, W, Wq, ero, s);
            cas_morph_launch(mid, res, D, H, W, Wq, dil, s);
            break;
    }
    if (check_launch("feed_cascade_morph")) return 1;
    hipLaunchKernelGGL(k_cas_apply, dim3(cas_grid(nwords)), dim3(256), 0, s, (u64 *)planes, res, K, c, nwords);
    return check_launch("feed_cascade_morph apply");
}

size_t mvd_feed_cascade_remove_workspace_bytes(long n) {
    if (n <= 0) return 0;
    return cas_align((size_t)n) + 2 * cas_align((size_t)n * sizeof(int32_t)) + 256 + 1024 * sizeof(int32_t);
}

int mvd_feed_cascade_remove(float *chan, float *other, int D, int H, int W, long threshold, double u, void *ws,
                            size_t ws_bytes, int32_t *chosen, void *stream) {
    MVD_REQUIRE(chan && ws && chosen, "feed_cascade_remove: null pointer");
    MVD_REQUIRE(cas_shape_ok(D, H, W), "feed_cascade_remove: bad shape");
    MVD_REQUIRE(u >= 0.0 && u < 1.0, "feed_cascade_remove: u in [0, 1)");
    MVD_REQUIRE(threshold >= 0, "feed_cascade_remove: threshold >= 0");
    const long n = (long)D * H * W;
    MVD_REQUIRE(ws_bytes >= mvd_feed_cascade_remove_workspace_bytes(n), "feed_cascade_remove: workspace too small");
    char *p = (char *)ws;
    uint8_t *mask = (uint8_t *)p;
    p += cas_align((size_t)n);
    int32_t *labels = (int32_t *)p;
    p += cas_align((size_t)n * sizeof(int32_t));
    int32_t *sizes = (int32_t *)p;
    p += cas_align((size_t)n * sizeof(int32_t));
    int32_t *count = (int32_t *)p;
    p += 256;
    int32_t *blockcnt = (int32_t *)p;
    const int32_t thr = (int32_t)(threshold > 2147483647L ? 2147483647L : threshold);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_cas_mask, dim3(cas_grid(n)), dim3(256), 0, s, chan, mask, n);
    if (check_launch("feed_cascade_remove mask")) return 1;
    if (mvd_cc_label(mask, labels, count, D, H, W, 26, stream)) return 1;
    if (mvd_cc_component_sizes(labels, sizes, n, stream)) return 1;
    const int nblocks = cas_blocks(n);
    const long chunk = cdiv(n, nblocks);
    hipLaunchKernelGGL(k_cas_count, dim3(nblocks), dim3(256), 0, s, sizes, n, chunk, thr, blockcnt);
    hipLaunchKernelGGL(k_cas_pick, dim3(1), dim3(256), 0, s, sizes, n, chunk, thr, blockcnt, nblocks, u, chosen);
    hipLaunchKernelGGL(k_cas_clear, dim3(cas_grid(n)), dim3(256), 0, s, labels, chan, other, n, chosen);
    return check_launch("feed_cascade_remove");
}
}
