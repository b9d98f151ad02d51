// bf16 mixed-precision forward-type conv engine (BASELINE cfg 4/5: bf16 activations, fp32 master weights and
// accumulation).  v_mfma_f32_32x32x16_bf16: A[row r][k = 8h+j], B[k = 8h+j][col r] (8 bf16 = one 16-byte fragment per
// lane and k-step), fp32 accumulate, 16x the fp32 MFMA rate -- at 32..64 output channels the kernel is bound by LDS /
// L2 bandwidth, not by the matrix pipe.
//
// Same gathered-tap GEMM as conv_mfma.hip (FwdGeom), C % 32 == 0, K % 32 == 0, any gather stride:
//   * activations NDHWC bf16: a 32-channel chunk of a voxel is 64 B; halo tile in LDS [slots][32 ch] padded to 80 B;
//   * packed weights bf16 [chunk][tap][s][h][k][8] (s = 16-channel k-step, h = lane half): the B fragment of lane
//     (r, h) is one 16-byte read; tap groups stream through a double-buffered LDS ring, next group prefetched into
//     registers under the current group's MFMAs;
//   * output bf16 (fp32 bias added in the epilogue); skinny problems split the reduce chunks and go through fp32
//     partials (k_split_reduce16).
#include <stdlib.h>

#include "common.h"
#include "conv_geom.h"

namespace mvd {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Epilogue store widening (guide T21): after a swapped-operand 32x32 MFMA chain lane (i, h) holds, per channel group
// rg, the packed bf16 x 4 of channels 8rg + 4h .. +3 of voxel i.  One v_permlane32_swap per dword turns the pair of
// groups (k, k+1) into 16 contiguous bytes per lane: lanes 0-31 get channels 8k .. 8k+7, lanes 32-63 channels
// 8k+8 .. 8k+15 -> one 16-byte store at byte offset 16k (+16 for the upper half) instead of two 8-byte ones.  The
// 8-byte stores are issue-bound (~7 B/clk/CU), not bandwidth-bound.
__device__ inline uint4 pair_store_image(uint2 a /* group k */, uint2 b /* group k+1 */) {
    auto rx = __builtin_amdgcn_permlane32_swap(a.x, b.x, false, false);
    auto ry = __builtin_amdgcn_permlane32_swap(a.y, b.y, false, false);
    return make_uint4(rx[0], ry[0], rx[1], ry[1]);
}
// img + old, element-wise on 8 packed bf16 (fp32 add, one rounding): the accumulate form of the epilogue (FwdGeom::acc)
__device__ inline uint4 add_bf16x8(uint4 a, uint4 b) {
    const unsigned av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
    unsigned r[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float lo = __uint_as_float(av[e] << 16) + __uint_as_float(bv[e] << 16);
        const float hi = __uint_as_float(av[e] & 0xffff0000u) + __uint_as_float(bv[e] & 0xffff0000u);
        r[e] = (unsigned)f2bf(lo) | ((unsigned)f2bf(hi) << 16);
    }
    return make_uint4(r[0], r[1], r[2], r[3]);
}
__device__ inline uint2 pack_bf16x4(float a, float b, float c, float d) {
    uint2 q;
    q.x = (unsigned)f2bf(a) | ((unsigned)f2bf(b) << 16);
    q.y = (unsigned)f2bf(c) | ((unsigned)f2bf(d) << 16);
    return q;
}

__host__ __device__ inline size_t widx16(int T, int K, int t, int c, int k) {
    const int cc = c >> 5, r = c & 31, s = r >> 4, h = (r >> 3) & 1, e = r & 7;
    return ((((((size_t)cc * T + t) * 2 + s) * 2 + h) * K + k) << 3) + e;
}

// torch fp32 [K][C][T] (or transposed-conv [C][K][T]) -> wf16 (reduce C, produce K) / wb16 (reduce K, produce C)
__global__ void k_pack_weight16(const float *__restrict__ w, unsigned short *__restrict__ wf, unsigned short *__restrict__ wb,
                                int K, int C, int T, int transposed) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)K * C * T;
    if (i >= total) return;
    int k = i % K;
    int c = (i / K) % C;
    int t = i / ((long)K * C);
    float v = transposed ? w[((size_t)c * K + k) * T + t] : w[((size_t)k * C + c) * T + t];
    unsigned short b = f2bf(v);
    if (wf) wf[widx16(T, K, t, c, k)] = b;
    if (wb) wb[widx16(T, C, t, k, c)] = b;
}

struct Fwd16Tile {
    int EH, EW, nslots;
    int magW, magHW;
    int min_off[3];
    int ntd, nth, ntw, nkb, S;
    int nitems;
    int K;
    int toff[27];
    signed char tdy[28];  // unused (read only by the removed XOR-swizzled halo layout); kept so the argument layout stays
};

// XR: uint4 (8 bf16) per thread of the halo tile = ceil(nslots*4/256)
// Halo slots are padded to 80 bytes: 3-way conflicted on unit-stride problems (PMC round 2: as many conflict cycles as
// access cycles), but the conflict-free XOR-swizzled 64-byte layout measured 12-15 % SLOWER here (two workgroups per CU:
// the kernel is bound by instruction issue, and the swizzle is arithmetic per read) and was removed.
template <int NT, int MT, int TG, int XR, int NW = 4>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void k_fwd16(const FwdGeom g, const Fwd16Tile tg, const unsigned short *__restrict__ a1,
                                                  const unsigned short *__restrict__ a2,
                                                  const unsigned short *__restrict__ w, const float *__restrict__ bias,
                                                  unsigned short *__restrict__ y1, unsigned short *__restrict__ y2,
                                                  float *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds8[];
    constexpr int KT = 32 * NT;
    constexpr int TPB = NW * 64;                 // threads: wave w owns output plane od0 + w of the NW x (4 MT) x 8 tile
    constexpr int XS = 80;                       // bytes per halo slot (64 + 16 pad)
    constexpr int WROW = 16;                     // bytes per (tap, s, h, k) weight fragment
    constexpr int WR = TG * 4 * KT / TPB;        // uint4 per thread per weight group (TG*2*2*KT fragments)
    constexpr int WBUF = TG * 4 * KT * WROW;     // bytes per weight buffer
    static_assert((TG * 4 * KT) % TPB == 0, "weight group must be a multiple of the thread count");
    unsigned char *Xs = lds8;
    unsigned char *Wsm = lds8 + (size_t)XR * (TPB / 4) * XS;  // halo buffer sized for XR*TPB/4 >= nslots slots
    // Per-tap tables across the lanes of a wave (round 2): lane t holds the halo byte offset of tap t and its index in
    // the packed weights; the loops read them back with v_readlane (a few cycles, result in an SGPR).  Indexed out of
    // the kernel argument they were an s_load (+ a byte load) per tap INSIDE the MFMA loop, each followed by
    // s_waitcnt lgkmcnt(0) -- SMEM returns out of order, so the wait also drained every operand read in flight.  (A
    // first fix kept the tables in LDS: in-kernel s_memtime stamps then showed the three weight loads of a group taking
    // ~900 cycles to ISSUE -- three serial LDS round trips, each in front of a 64-bit address computation.)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int per_xcd = (tg.nitems + 7) >> 3;
    const int item = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (item >= tg.nitems) return;
    unsigned r_ = (unsigned)item;
    const int kb = (int)(r_ % (unsigned)tg.nkb); r_ /= (unsigned)tg.nkb;
    const int split = (int)(r_ % (unsigned)tg.S); r_ /= (unsigned)tg.S;
    const int tw_ = (int)(r_ % (unsigned)tg.ntw); r_ /= (unsigned)tg.ntw;
    const int th_ = (int)(r_ % (unsigned)tg.nth); r_ /= (unsigned)tg.nth;
    const int td_ = (int)(r_ % (unsigned)tg.ntd);
    const int n = (int)(r_ / (unsigned)tg.ntd);

    const int ltc = lane < g.ntaps ? lane : g.ntaps - 1;
    const int toff_l = tg.toff[ltc < 27 ? ltc : 26] * XS;                 // (clamped to the last tap beyond ntaps)
    const int wt_l = (int)g.wt[ltc < 27 ? ltc : 26];  // (slots past the last tap load the last tap's weights: their MFMAs are skipped)
    const int C = g.C1 + g.C2;
    const int nch = C / 32;
    const int ngroups = (g.ntaps + TG - 1) / TG;
    const int EHW = tg.EH * tg.EW;
    const int nx = tg.nslots * 4;
    const int od0 = td_ * NW, oh0 = th_ * (4 * MT), ow0 = tw_ * 8;
    const int iz0 = od0 * g.sa[0] + tg.min_off[0], iy0 = oh0 * g.sa[1] + tg.min_off[1], ix0 = ow0 * g.sa[2] + tg.min_off[2];

    int sbase[MT];
#pragma unroll
    for (int m = 0; m < MT; m++)
        sbase[m] = (((wave * g.sa[0]) * tg.EH + (4 * m + (i >> 3)) * g.sa[1]) * tg.EW + (i & 7) * g.sa[2]) * XS + h * 16;
    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int q = 0; q < NT; q++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[m][q][r] = 0.f;

    // weight group: fragment index f = u*256 + tid = ((tl*2 + s)*2 + hh)*KT + k ; tl is a compile-time function of u
    uint4 wrA[WR], wrB[WR];  // two groups of weights in flight (round 2): a group's loads have two groups of MFMAs to land
#pragma unroll
    for (int u = 0; u < WR; u++) wrA[u] = wrB[u] = make_uint4(0, 0, 0, 0);  // (defined on every path: stays in registers)
    unsigned woff[WR];
    constexpr int FPT = 4 * KT;  // fragments per tap
#pragma unroll
    for (int u = 0; u < WR; u++) {
        const int f = (u * TPB + tid) % FPT;
        const int k = f % KT, sh = f / KT;  // sh = s*2 + hh
        woff[u] = (unsigned)((sh * tg.K + kb * KT + k) * 16);  // BYTE offset inside a (chunk, tap) block of 4*K*8 elements
    }
    auto load_w = [&](int cc, int gidx, uint4(&dst)[WR]) {
#pragma unroll
        for (int u = 0; u < WR; u++) {
            // tap of slot u: FPT = 256 -> u; FPT = 128 -> 2u + (tid >> 7): uniform per wave either way
            const int t = __builtin_amdgcn_readfirstlane(gidx * TG + (u * TPB + tid) / FPT);  // < 32
            const int wt = __builtin_amdgcn_readlane(wt_l, t);
            // unconditional: with a branch around the load the compiler loses the vmcnt count and waits for vmcnt(0) in
            // front of every weight store -- i.e. also for the group that was requested last.  Scalar base + 32-bit lane
            // offset (the empty asm keeps the zero-extension next to the load: saddr addressing instead of a 64-bit
            // multiply-add per load -- ~30 instructions per load made the three loads of a group take ~500 cycles to issue)
            const char *wb_ = reinterpret_cast<const char *>(w + ((size_t)cc * g.T + wt) * 4 * tg.K * 8);
            asm volatile("" : "+v"(woff[u]));
            dst[u] = *reinterpret_cast<const uint4 *>(wb_ + woff[u]);
        }
    };
    auto store_w = [&](int buf, const uint4(&src)[WR]) {
#pragma unroll
        for (int u = 0; u < WR; u++)
            *reinterpret_cast<uint4 *>(Wsm + (size_t)buf * WBUF + (size_t)(u * TPB + tid) * WROW) = src[u];
    };

    const int cc_begin = split * nch / tg.S, cc_end = (split + 1) * nch / tg.S;
    // every workgroup streams the same few hundred KB of weights from L2, and workgroups launched together walk them in
    // step: the tap groups are taken in an order rotated by the work item, so that at any time the CUs of an XCD ask for
    // different lines (ablation round 2: the weight path was 64 of the 118 us this kernel needs WITHOUT its MFMAs on
    // 64 -> 64 @64^3 -- 450 MB of L2 reads per launch)
    // halo of one 32-channel chunk into registers (XR x 16 bytes per thread)
    constexpr bool PREF = NW == 8;
    uint4 hv[XR];
    auto load_halo = [&](int cc) {
        const int c0 = cc * 32;
        const unsigned short *src;
        int Cs, cofs;
        if (c0 < g.C1) {
            src = a1; Cs = g.C1; cofs = c0;
        } else {
            src = a2; Cs = g.C2; cofs = c0 - g.C1;
        }
#pragma unroll
        for (int u = 0; u < XR; u++) {
            const int idx = u * TPB + tid;
            hv[u] = make_uint4(0, 0, 0, 0);
            if (idx < nx) {
                const int slot = idx >> 2;
                const int ez = (slot * tg.magHW) >> 20, rem = slot - ez * EHW;
                const int ey = (rem * tg.magW) >> 20, ex = rem - ey * tg.EW;
                const int id = iz0 + ez, ih = iy0 + ey, iw = ix0 + ex;
                if (id >= 0 && id < g.Di && ih >= 0 && ih < g.Hi && iw >= 0 && iw < g.Wi)
                    hv[u] = *reinterpret_cast<const uint4 *>(
                        src + ((((size_t)n * g.Di + id) * g.Hi + ih) * g.Wi + iw) * Cs + cofs + (tid & 3) * 8);
            }
        }
    };
    const int rot = item % ngroups;
    const bool fullg = ngroups * TG == g.ntaps;  // every group has TG taps (27 taps, TG = 3): no per-slot tap tests
    for (int cc = cc_begin; cc < cc_end; cc++) {
        load_w(cc, rot, wrA);
        if (ngroups > 1) load_w(cc, (rot + 1) % ngroups, wrB);
        if (!PREF || cc == cc_begin) load_halo(cc);
        __syncthreads();  // B1: every wave is done with the previous chunk's LDS
#pragma unroll
        for (int u = 0; u < XR; u++) {
            const int idx = u * TPB + tid;
            *reinterpret_cast<uint4 *>(Xs + (size_t)(idx >> 2) * XS + (idx & 3) * 16) = hv[u];
        }
        // PREF (one workgroup per CU: nothing else hides the fetch): the next chunk's halo travels while this chunk's 27 taps run
        if (PREF && cc + 1 < cc_end) load_halo(cc + 1);
        auto group_mfmas = [&](int gi, int wbuf) __attribute__((always_inline)) {
            const unsigned char *wb_ = Wsm + (size_t)wbuf * WBUF;
            // operand registers are double buffered over the 2*TG (tap, k-step) slots of the group: the fragments of
            // slot j+1 are read from LDS before slot j's MFMAs are issued, so a register an in-flight MFMA still reads
            // is never the target of the next ds_read (tools/probes/mfma_probe.hip: 111 -> 137 TFLOP/s effect)
            // RA = read-ahead in (tap, k-step) slots.  (Round 3: RA = 2 on the eight-wave form -- a slot is only four MFMAs per
            // wave -- measured SLOWER: 128 -> 128 @32^3 0.070 -> 0.071, 256 -> 128 0.118 -> 0.125 ms.)
            constexpr int RA = 1, NBUF = RA + 1;
            bf16x8 af[NBUF][MT], bfr[NBUF][NT];
            int to3[TG];
#pragma unroll
            for (int tl = 0; tl < TG; tl++) to3[tl] = __builtin_amdgcn_readlane(toff_l, gi * TG + tl);
            auto read_ops = [&](int j, int buf) {
                const int tl = j >> 1, s = j & 1;
                const int to = to3[tl];
                const int xo = s * 32;
#pragma unroll
                for (int m = 0; m < MT; m++) {
                    uint4 q = *reinterpret_cast<const uint4 *>(Xs + sbase[m] + to + xo);
                    af[buf][m] = *reinterpret_cast<bf16x8 *>(&q);
                }
#pragma unroll
                for (int q_ = 0; q_ < NT; q_++) {
                    uint4 q = *reinterpret_cast<const uint4 *>(wb_ + ((size_t)((tl * 2 + s) * 2 + h) * KT + q_ * 32 + i) * WROW);
                    bfr[buf][q_] = *reinterpret_cast<bf16x8 *>(&q);
                }
            };
#pragma unroll
            for (int j = 0; j < RA && j < 2 * TG; j++) read_ops(j, j % NBUF);
#pragma unroll
            for (int j = 0; j < 2 * TG; j++) {
                if (j + RA < 2 * TG) read_ops(j + RA, (j + RA) % NBUF);
                if (fullg || gi * TG + (j >> 1) < g.ntaps) {  // block-uniform
#pragma unroll
                    for (int m = 0; m < MT; m++)
#pragma unroll
                        for (int q_ = 0; q_ < NT; q_++)
                            acc[m][q_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bfr[j % NBUF][q_], af[j % NBUF][m], acc[m][q_], 0, 0, 0);
                }
            }
        };
        // group gi: its weights (loaded two groups ago into register set gi & 1) go to LDS buffer gi & 1 -- last read by
        // group gi-2, which every wave left before the barrier of group gi-1 -- and the freed registers take group gi+2.
        // With one register set the loads of group gi+1 had only group gi's 24 MFMAs (~0.4 us) to come back from L2.
        int gr = rot, gr2 = rot + 2 >= ngroups ? rot + 2 - ngroups : rot + 2;  // rotated indices of groups gj and gj + 2
        if (gr2 >= ngroups) gr2 -= ngroups;                                     // (ngroups == 1)
        // one group: PAR = its LDS buffer / register set (two named arrays: an array of arrays went to scratch memory)
#define MVD_F16_GROUP(PAR, WRX)                                  \
        {                                                        \
            store_w(PAR, WRX);                                   \
            __syncthreads(); /* B2 */                            \
            if (gj + 2 < ngroups) load_w(cc, gr2, WRX);          \
            group_mfmas(gr, PAR);                                \
            gr = gr + 1 == ngroups ? 0 : gr + 1;                 \
            gr2 = gr2 + 1 == ngroups ? 0 : gr2 + 1;              \
        }
        for (int gj = 0; gj < ngroups;) {
            MVD_F16_GROUP(0, wrA)
            if (++gj >= ngroups) break;
            MVD_F16_GROUP(1, wrB)
            ++gj;
        }
#undef MVD_F16_GROUP
    }
    // epilogue.  The MFMA operands are swapped (D^T = W^T X^T): column (lane & 31) = voxel of the M tile, rows = output
    // channels (r & 3) + 8 * (r >> 2) + 4 * h -- a lane holds 4 x 4 consecutive channels of ONE voxel and stores them as
    // 8-byte bf16 packets (sixteen 2-byte stores per tile cost more than the tile's MFMAs)
    const int od = od0 + wave;
    if (od >= g.Do) return;  // wave-uniform
    // the tile's bias values first, settled (common.h): loads between the stores would serialise them
    float4 bq[NT][4];
#pragma unroll
    for (int q = 0; q < NT; q++)
#pragma unroll
        for (int rg = 0; rg < 4; rg++)
            bq[q][rg] = (bias && tg.S == 1) ? *reinterpret_cast<const float4 *>(bias + kb * KT + q * 32 + 8 * rg + 4 * h)
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < NT; q++)
#pragma unroll
        for (int rg = 0; rg < 4; rg++) bq[q][rg] = settled(bq[q][rg]);
#pragma unroll
    for (int m = 0; m < MT; m++) {
        const int oh = oh0 + 4 * m + (i >> 3), ow = ow0 + (i & 7);
        const bool inside = oh < g.Ho && ow < g.Wo;  // (every lane takes part in the lane-half exchange below)
        const size_t o_lin = ((size_t)od * g.Ho + oh) * g.Wo + ow;
        const size_t ov = (((size_t)n * g.Dy + (od * g.so[0] + g.oo[0])) * g.Hy + (oh * g.so[1] + g.oo[1])) * g.Wy +
                          (ow * g.so[2] + g.oo[2]);
#pragma unroll
        for (int q = 0; q < NT; q++) {
            if (tg.S > 1) {
#pragma unroll
                for (int rg = 0; rg < 4; rg++) {
                    const int k = kb * KT + q * 32 + 8 * rg + 4 * h;
                    if (inside)
                        *reinterpret_cast<float4 *>(part + (((size_t)split * g.N + n) * ((size_t)g.Do * g.Ho * g.Wo) + o_lin) * tg.K + k) =
                            make_float4(acc[m][q][rg * 4 + 0], acc[m][q][rg * 4 + 1], acc[m][q][rg * 4 + 2], acc[m][q][rg * 4 + 3]);
                }
            } else {
#pragma unroll
                for (int kp = 0; kp < 2; kp++) {  // channel groups 2kp, 2kp+1: one 16-byte store per lane (T21)
                    uint2 pk[2];
#pragma unroll
                    for (int e = 0; e < 2; e++) {
                        const int rg = 2 * kp + e;
                        const float4 b4 = bq[q][rg];
                        pk[e] = pack_bf16x4(acc[m][q][rg * 4 + 0] + b4.x, acc[m][q][rg * 4 + 1] + b4.y,
                                            acc[m][q][rg * 4 + 2] + b4.z, acc[m][q][rg * 4 + 3] + b4.w);
                    }
                    const uint4 img = pair_store_image(pk[0], pk[1]);
                    const int k = kb * KT + q * 32 + 16 * kp + 8 * h;  // first of this lane's 8 consecutive channels
                    if (inside) {
                        if (k < g.K1) {
                            uint4 *dst = reinterpret_cast<uint4 *>(y1 + ov * g.K1 + k);
                            *dst = g.acc ? add_bf16x8(img, *dst) : img;   // (block-uniform)
                        } else
                            *reinterpret_cast<uint4 *>(y2 + ov * g.K2 + (k - g.K1)) = img;
                    }
                }
            }
        }
    }
}

// y[mapped(n,o)][k] = bf16( bias[k] + sum_s part[s][n][o][k] )
__global__ void k_split_reduce16(const FwdGeom g, const float *__restrict__ part, const float *__restrict__ bias,
                                 unsigned short *__restrict__ y1, unsigned short *__restrict__ y2, int S) {
    const int K = g.K1 + g.K2;
    const size_t per = (size_t)g.N * g.Do * g.Ho * g.Wo * K;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < per; idx += (size_t)gridDim.x * blockDim.x) {
        float s = bias ? bias[idx % K] : 0.f;
        int j = 0;
        for (; j + 3 < S; j += 4) {  // four partials in flight, added in split order (same sum as one at a time)
            const float p0 = part[(size_t)j * per + idx], p1 = part[(size_t)(j + 1) * per + idx];
            const float p2 = part[(size_t)(j + 2) * per + idx], p3 = part[(size_t)(j + 3) * per + idx];
            s += p0;
            s += p1;
            s += p2;
            s += p3;
        }
        for (; j < S; j++) s += part[(size_t)j * per + idx];
        const int k = (int)(idx % K);
        size_t r = idx / K;
        const int ow = (int)(r % g.Wo);
        r /= g.Wo;
        const int oh = (int)(r % g.Ho);
        r /= g.Ho;
        const int od = (int)(r % g.Do);
        const int n = (int)(r / g.Do);
        const size_t ov = (((size_t)n * g.Dy + (od * g.so[0] + g.oo[0])) * g.Hy + (oh * g.so[1] + g.oo[1])) * g.Wy +
                          (ow * g.so[2] + g.oo[2]);
        if (k < g.K1)
            y1[ov * g.K1 + k] = f2bf(g.acc ? s + __uint_as_float((unsigned)y1[ov * g.K1 + k] << 16) : s);
        else
            y2[ov * g.K2 + (k - g.K1)] = f2bf(s);
    }
}

// ------------------------------------------------------------------------------------------------ stride-2 input gradient
// bf16 twin of k_dgrad32s (conv_mfma.hip): dx of a 3x3x3 stride-2 pad-1 conv, all eight output-parity classes from ONE
// staged dy tile.  The per-class launches of the gather engine re-read dy eight times and run 1- and 2-tap classes as whole
// launches (0.37 ms for 64 -> 32 at 128^3, whose traffic and MFMA work are ~0.07 ms each).  Workgroup = 8 waves on a
// 3 x 5 x 9 dy tile (2 x 4 x 8 positions j + the odd classes' +1 neighbours) per 32-channel reduce chunk; wave w takes
// class w on the positions of plane oz0 and class 7 - w on plane oz0 + 1 (6 or 9 tap groups per wave).  Swapped product
// D^T = W^T dy^T on v_mfma_f32_32x32x16_bf16: A = packed weights straight from L2 (one tap ahead), B = dy fragment from the
// LDS tile ([slot][64 B], 16-byte parts XORed by (slot >> 2) & 3: 2-way conflicts at worst); a lane ends with 16
// channels of ONE dx voxel and stores two 16-byte images (permlane32 exchange).  FwdGeom::acc adds into dx.
struct Dg16Tile {
    int ntd, nth, ntw, ncb, nitems, C;
    int acc;
};
__global__ __launch_bounds__(512, 2) void k_dgrad16s(const FwdGeom g, const Dg16Tile tg, const unsigned short *__restrict__ dy,
                                                     const unsigned short *__restrict__ wb, unsigned short *__restrict__ dx) {
    __shared__ __attribute__((aligned(16))) unsigned char Xs[135 * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int per_xcd = (tg.nitems + 7) >> 3;
    const int item = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (item >= tg.nitems) return;
    unsigned r_ = (unsigned)item;
    const int cb = (int)(r_ % (unsigned)tg.ncb); r_ /= (unsigned)tg.ncb;
    const int tw_ = (int)(r_ % (unsigned)tg.ntw); r_ /= (unsigned)tg.ntw;
    const int th_ = (int)(r_ % (unsigned)tg.nth); r_ /= (unsigned)tg.nth;
    const int td_ = (int)(r_ % (unsigned)tg.ntd);
    const int n = (int)(r_ / (unsigned)tg.ntd);
    // g.Di/Hi/Wi = dy grid (conv output), g.Dy/Hy/Wy = dx grid (conv input), g.C1 = K (reduce), tg.C = channels of dx
    const int K = g.C1, C = tg.C;
    const int nch = K >> 5;
    const int oz0 = td_ * 2, oy0 = th_ * 4, ox0 = tw_ * 8;
    // packed dgrad weights [chunk][tap][s][h][c][8]: lane (c = i, h) of k-step s
    const unsigned short *wlane = wb + ((size_t)h * C + cb * 32 + i) * 8;
    const size_t wstep = (size_t)2 * C * 8, wtap = 2 * wstep;
    f32x16 acc[2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[m][r] = 0.f;
    for (int kk = 0; kk < nch; kk++) {
        __syncthreads();
        {
            const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<unsigned short *>(dy + (size_t)n * g.Di * g.Hi * g.Wi * K + kk * 32), 0, 0x7fffffff, 0x00020000);
            uint4 v[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int idx = tid + u * 512;
                const int slot = idx >> 2, part = idx & 3;
                const int ez = slot / 45, rem = slot - ez * 45;
                const int ey = rem / 9, ex = rem - ey * 9;
                const int oz = oz0 + ez, oy = oy0 + ey, ox = ox0 + ex;
                const bool ok = idx < 135 * 4 && oz < g.Di && oy < g.Hi && ox < g.Wi;
                const unsigned o = ok ? (unsigned)(((oz * g.Hi + oy) * g.Wi + ox) * K + part * 8) * 2u : 0xffffffffu;
                v[u] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rdy, (int)o, 0, 0));
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int idx = tid + u * 512;
                const int slot = idx >> 2, part = idx & 3;
                if (idx < 135 * 4) *reinterpret_cast<uint4 *>(Xs + slot * 64 + ((part ^ ((slot >> 2) & 3)) << 4)) = v[u];
            }
        }
        __syncthreads();
        const unsigned short *wc = wlane + (size_t)kk * 27 * wtap;
#pragma unroll
        for (int m = 0; m < 2; m++) {
            const int q = m ? 7 - wave : wave;
            const int pz = q >> 2, py = (q >> 1) & 1, px = q & 1;
            const int slot0 = (m * 5 + (i >> 3)) * 9 + (i & 7);
            // the class's taps: per axis (t = 1, d = 0) for an even coordinate, (t = 0, d = 1) and (t = 2, d = 0) for an odd one
            const int ntq = 1 << (pz + py + px);
            auto tap_of = [&](int j, int &t, int &so) {
                const int bz = pz ? (j >> (py + px)) & 1 : 0, by = py ? (j >> px) & 1 : 0, bx = px ? j & 1 : 0;
                const int tz = pz ? (bz ? 2 : 0) : 1, ty = py ? (by ? 2 : 0) : 1, tx = px ? (bx ? 2 : 0) : 1;
                const int dz = (pz && !bz) ? 1 : 0, dyy = (py && !by) ? 1 : 0, dxx = (px && !bx) ? 1 : 0;
                t = (tz * 3 + ty) * 3 + tx;
                so = (dz * 5 + dyy) * 9 + dxx;
            };
            uint4 wv[2][2];
            int t0, so0;
            tap_of(0, t0, so0);
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) wv[0][s2] = *reinterpret_cast<const uint4 *>(wc + (size_t)t0 * wtap + s2 * wstep);
            for (int j = 0; j < ntq; j += 2) {  // two taps per trip: static buffer indices (ntq is 1, 2, 4 or 8)
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    if (j + u < ntq) {  // wave-uniform
                        int t, so, tn, son;
                        tap_of(j + u, t, so);
                        tap_of(j + u + 1 < ntq ? j + u + 1 : j + u, tn, son);
#pragma unroll
                        for (int s2 = 0; s2 < 2; s2++)
                            wv[(u + 1) & 1][s2] = *reinterpret_cast<const uint4 *>(wc + (size_t)tn * wtap + s2 * wstep);
                        const int slot = slot0 + so;
#pragma unroll
                        for (int s2 = 0; s2 < 2; s2++) {
                            const uint4 xq = *reinterpret_cast<const uint4 *>(Xs + slot * 64 + ((((s2 << 1) | h) ^ ((slot >> 2) & 3)) << 4));
                            acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8 *>(&wv[u][s2]),
                                                                            *reinterpret_cast<const bf16x8 *>(&xq), acc[m], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    // lane (i, h) holds, per M tile m, channels (r & 3) + 8 (r >> 2) + 4 h of dx voxel 2 j + p, j = (oz0 + m, oy0 + (i >> 3),
    // ox0 + (i & 7)): two 16-byte images after the lane-half exchange
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const int q = m ? 7 - wave : wave;
        const int pz = q >> 2, py = (q >> 1) & 1, px = q & 1;
        const int iz = 2 * (oz0 + m) + pz, iy = 2 * (oy0 + (i >> 3)) + py, ix = 2 * (ox0 + (i & 7)) + px;
        const bool inside = iz < g.Dy && iy < g.Hy && ix < g.Wy;
        const size_t ov = (((size_t)n * g.Dy + iz) * g.Hy + iy) * g.Wy + ix;
#pragma unroll
        for (int kp = 0; kp < 2; kp++) {
            uint2 pk[2];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int rg = 2 * kp + e;
                pk[e] = pack_bf16x4(acc[m][rg * 4 + 0], acc[m][rg * 4 + 1], acc[m][rg * 4 + 2], acc[m][rg * 4 + 3]);
            }
            const uint4 img = pair_store_image(pk[0], pk[1]);
            if (inside) {
                uint4 *dst = reinterpret_cast<uint4 *>(dx + ov * C + cb * 32 + 16 * kp + 8 * h);
                *dst = tg.acc ? add_bf16x8(img, *dst) : img;
            }
        }
    }
}

// (Round 3, tried: a persistent form for K <= 64 -- one workgroup per CU walking tiles, the wave's class weights resident in
// 128 registers, the next tile's dy prefetched into registers: 64 -> 32 at 128^3 0.189 -> 0.179 ms, nothing inside the step.
// The launch is bound by one memory round trip per 49 KB tile with two tiles in flight per CU either way, not by the
// weights' L2 latency; more tiles in flight do not fit beside resident weights.  Not kept.)
int dgrad16s(int N, int D, int H, int W, int C, int K, int Do, int Ho, int Wo, const unsigned short *dy, const unsigned short *wb,
             unsigned short *dx, hipStream_t s, int accumulate) {
    static const int on = getenv("MVD_DGRAD16S") ? atoi(getenv("MVD_DGRAD16S")) : 1;
    if (!on || C % 32 || K % 32 || (((uintptr_t)dy | (uintptr_t)wb | (uintptr_t)dx) & 15)) return -1;
    if ((long)Do * Ho * Wo * K * 2 >= (1L << 31)) return -1;  // 32-bit byte offsets inside one sample of dy (buffer loads)
    FwdGeom g;
    memset(&g, 0, sizeof(g));
    g.N = N;
    g.Di = Do; g.Hi = Ho; g.Wi = Wo;
    g.Dy = D; g.Hy = H; g.Wy = W;
    g.C1 = K;
    Dg16Tile tg;
    tg.ntd = (Do + 1) / 2; tg.nth = (Ho + 3) / 4; tg.ntw = (Wo + 7) / 8;
    tg.ncb = C / 32;
    tg.C = C;
    tg.acc = accumulate;
    const long nitems = (long)N * tg.ntd * tg.nth * tg.ntw * tg.ncb;
    if (nitems > (1L << 30)) return -1;
    tg.nitems = (int)nitems;
    const unsigned grid = (unsigned)(((nitems + 7) / 8) * 8);
    hipLaunchKernelGGL(k_dgrad16s, dim3(grid), dim3(512), 0, s, g, tg, dy, wb, dx);
    return check_launch("conv dgrad bf16 (stride 2, fused parity classes)");
}

static const size_t LDS_LIMIT16 = 160 * 1024;

template <int NT, int MT, int TG, int XR, int NW = 4>
static int launch_fwd16(const FwdGeom &g, Fwd16Tile &tg, const unsigned short *a1, const unsigned short *a2,
                        const unsigned short *w, const float *bias, unsigned short *y1, unsigned short *y2, void *ws,
                        size_t ws_bytes, hipStream_t s) {
    auto kern = k_fwd16<NT, MT, TG, XR, NW>;
    const size_t lds = (size_t)XR * (NW * 16) * 80 + 2 * (size_t)TG * 4 * (32 * NT) * 16 + 256;  // + tap tables
    if (lds > LDS_LIMIT16) return -1;
    static PerDeviceFlag configured;
    if (!configured()) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)LDS_LIMIT16) != hipSuccess) {
            set_error("conv fwd16: cannot raise the dynamic LDS limit");
            return 1;
        }
        configured() = true;
    }
    const int K = g.K1 + g.K2;
    tg.nkb = K / (32 * NT);
    const long tiles = (long)tg.ntd * tg.nth * tg.ntw;
    const size_t out_elems = (size_t)g.N * g.Do * g.Ho * g.Wo * K;
    const long wgs = tiles * tg.nkb * g.N;
    const int nch = (g.C1 + g.C2) / 32;
    int S = 1;
    if (ws && wgs < 256 && nch >= 4) {
        long want = (512 + wgs - 1) / wgs;
        if (want > 16) want = 16;
        if (want > nch / 2) want = nch / 2;
        while (want > 1 && (size_t)want * out_elems * sizeof(float) > ws_bytes) want--;
        if (want > 1) S = (int)want;
    }
    tg.S = S;
    const long nitems = tiles * tg.nkb * tg.S * g.N;
    if (nitems > (1L << 30)) return -1;
    tg.nitems = (int)nitems;
    const long grid = ((nitems + 7) / 8) * 8;
    float *part = reinterpret_cast<float *>(ws);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NW * 64), lds, s, g, tg, a1, a2, w, bias, y1, y2, part);
    if (check_launch("conv fwd16 (bf16 mfma)")) return 1;
    if (S > 1) {
        long blocks = cdiv((long)out_elems, 256);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(k_split_reduce16, dim3(blocks), dim3(256), 0, s, g, part, bias, y1, y2, S);
        return check_launch("conv fwd16 split reduce");
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ k_fwd16z (round 2)
// z-marching form of the 32 -> 32 channel 3x3x3 stride-1 convolution at high resolution (enc0.conv1, dec5.conv1 and their
// input gradients: 537 MB of activations, 232 GFLOP each).  Its persistent tile-walking predecessors (DESIGN.md 3.4, 9.5;
// removed) were bound by the traffic a 4x8x8 tile pulls through the CU's vector-memory pipe (a 6x10x10 halo: 2.34 bytes
// fetched per byte used) with one wave per SIMD to issue it.  Here a workgroup owns an 8 x 32 (y, x) column and walks a
// chunk of z-planes:
//   * input plane z' arrives once (10 x 34 voxels: 1.33 bytes fetched per byte used, rows of 2 KB contiguous in HBM),
//     register-staged (two planes in flight: loaded three planes ahead of its MFMAs -- one plane ahead left the loaded
//     HBM latency exposed) into a ring of four LDS plane images;
//   * every A fragment read from LDS (input row r, x shift dx, k-step) feeds up to SIX MFMAs: the three dz taps -- they
//     accumulate into three different OUTPUT planes z'+1, z', z'-1, held as a ring of four accumulator sets, so no
//     partial sum ever moves -- times the one or two M tiles (output rows) of the wave that see row r at some dy:
//     24 ds_read_b128 per 108 MFMAs (one read per MFMA in the tile walk);
//   * a wave = two M tiles (two output rows of 32 voxels); a workgroup is 4 waves (one per SIMD, 512 registers each) and
//     every lane keeps ALL 27 taps' B fragments (54 16-byte weight fragments, 216 registers) in the accumulator half of
//     the register file for the whole walk, where the MFMA reads them (inline asm: with the builtin hipcc copies each one
//     to a VGPR before use); the plane loop is unrolled four times so that ring positions are register names and LDS
//     offsets are immediates;
//   * the output plane completed by plane z' is converted between the MFMAs of plane z'+1 (fourth set), transposed
//     through a 4-KB per-wave LDS scratch and stored as four fully contiguous 1-KB wave stores; the drained set is then
//     re-initialised with the bias from an LDS table (ds_read_b128 straight into the accumulator registers).
// With one wave per SIMD nothing hides behind another wave: everything that is not an MFMA is either precomputed per
// column (the column is fixed for the life of the workgroup), an immediate, a range-checked buffer access (zeros outside
// the plane / dropped stores: no selects, no branches) or dealt out over the 24 fragment slots of a plane.
// A-operand LDS image of a plane: two sub-images (k-step 0: channels 0-15, k-step 1: 16-31) of 340 slots x 32 bytes; the
// two 16-byte halves of a slot are swapped when (slot >> 3) & 1: the 16 lanes of a ds_read_b128 group ({0-3,12-15,20-27},
// ...) read slots whose (slot mod 8) picks the 32-byte column of the 256-byte bank row, and the two lanes that share a
// column are 8 or 24 slots apart -- conflict-free for every dx; the k-step is an immediate offset.
constexpr int Z_ROWS = 10, Z_SLOTS = 34, Z_NSLOT = Z_ROWS * Z_SLOTS, Z_XR = 6, Z_PARTS = Z_NSLOT * 4;
constexpr int Z_HALF = Z_NSLOT * 32 + 64;      // +64: the two sub-images of a slot pair land on different write banks
constexpr int Z_PLANE = Z_HALF + Z_NSLOT * 32;
constexpr int Z_SCR = 4 * Z_PLANE, Z_BIAS = Z_SCR + 4 * 4096, Z_LDS = Z_BIAS + 4096;
static_assert(Z_PLANE + Z_HALF < 65536, "plane / k-step offsets must fit the 16-bit ds_read immediate");

struct Fwd16ZTile {
    int nty, ntx, nzc, zc, nitems;
    int kp, koff;  // produce channels of the packed weight tensor (its row stride), first produce channel of this launch
    int wsel[27];
};

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) u32x4 lds_u4;
typedef __attribute__((address_space(3))) u32x2 lds_u2;
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
__device__ inline unsigned cvt_pk_bf16(float a, float b) {  // one v_cvt_pk_bf16_f32 (round-to-nearest-even, as f2bf)
    f32x2 v = {a, b};
    bf16x2v r = __builtin_convertvector(v, bf16x2v);
    return *reinterpret_cast<unsigned *>(&r);
}

// A fragments come straight from ds_read_b128 (no VALU-written operand): no wait states needed in front of the MFMA
#define MVD_MFMA16_ZV(ACC, BFRAG, AFRAG) \
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(ACC) : "a"(BFRAG), "v"(AFRAG))

template <int R>
struct ZIdx { static constexpr int value = R; };

// FUSE (round 3, the InstanceNorm fusion of the north_star's block): bit 0 = statistics epilogue -- every 16-byte chunk
// of a finished output plane that passes through the store path (8 bf16 channels of one voxel per lane, the lane's
// channel octet fixed) is also accumulated into per-lane (sum, sum of squares) registers; one cross-lane / cross-wave
// combine at the end of the kernel writes the workgroup's partial [32 channels][2] (fixed order: deterministic).
// bit 1 = input prologue -- the staged input is the RAW output of the producing conv and is normalised + activated
// between the buffer load and the LDS write: a = bf16(lrelu(fma(x, scale[n][c], shift[n][c]))), zeros where the voxel
// lies outside the volume (the zero padding applies to the activation).
template <int FUSE = 0>
__global__ __launch_bounds__(256, 1) void k_fwd16z(const FwdGeom g, const Fwd16ZTile tg, const unsigned short *__restrict__ a1,
                                                   const unsigned short *__restrict__ w, const float *__restrict__ bias,
                                                   unsigned short *__restrict__ y1, float *__restrict__ tile_stats,
                                                   const float *__restrict__ in_scale, const float *__restrict__ in_shift,
                                                   const float slope) {
    constexpr bool PRO = (FUSE & 2) != 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds8[];
    const unsigned lbase = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)lds8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    // XCD-aware item order: each XCD walks a contiguous range of (n, chunk, ty, tx) -- neighbours share halo rows in its L2
    const int per_xcd = (tg.nitems + 7) >> 3;
    const int item = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= per_xcd || item >= tg.nitems) return;
    unsigned r_ = (unsigned)item;
    const int tx = (int)(r_ % (unsigned)tg.ntx); r_ /= (unsigned)tg.ntx;
    const int ty = (int)(r_ % (unsigned)tg.nty); r_ /= (unsigned)tg.nty;
    const int zchunk = (int)(r_ % (unsigned)tg.nzc);
    const int n_ = (int)(r_ / (unsigned)tg.nzc);
    const int y0 = ty * 8, x0 = tx * 32, zb = zchunk * tg.zc;
    const int ze = min(zb + tg.zc, g.Do);

    i32x4 bw[27][2];
#pragma unroll
    for (int p = 0; p < 27; p++)
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++) {
            const uint4 q = *reinterpret_cast<const uint4 *>(
                w + ((size_t)((tg.wsel[p] * 2 + s2) * 2 + h) * tg.kp + tg.koff + i) * 8);
            bw[p][s2] = *reinterpret_cast<const i32x4 *>(&q);
        }
    // staging slots (column constants): byte offset inside an input plane -- 0xfffffff0 for parts outside the (y, x) plane:
    // the plane is read through a buffer descriptor whose range check returns zeros there (no select, no branch) -- and
    // the LDS offset
    unsigned rel[Z_XR], wa[Z_XR];
#pragma unroll
    for (int u = 0; u < Z_XR; u++) {
        const int idx = u * 256 + tid;
        const int slot = idx < Z_PARTS ? (idx >> 2) : 0;
        const int ry = slot / Z_SLOTS, sx = slot - ry * Z_SLOTS;
        const int gy = y0 - 1 + ry, gx = x0 - 1 + sx;
        const bool in = idx < Z_PARTS && gy >= 0 && gy < g.Hi && gx >= 0 && gx < g.Wi;
        const int part = idx & 3;
        rel[u] = in ? (unsigned)((gy * g.Wi + gx) * 64 + part * 16) : 0xfffffff0u;
        wa[u] = lbase + (part >> 1) * Z_HALF + slot * 32 + (((part & 1) ^ ((slot >> 3) & 1)) << 4);
    }
#pragma unroll
    for (int u = 0; u < Z_XR; u++) asm volatile("" : "+v"(rel[u]), "+v"(wa[u]));  // one register each, no re-derivation per plane
    // A-operand read addresses: input row r of this wave, x shift dx (k-step and image parity are immediates; images 2, 3
    // lie beyond the 16-bit immediate: one v_add per read there -- a second set of 12 address registers spilled)
    unsigned ra[4][3];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int dx = 0; dx < 3; dx++) {
            const int slot = (2 * wave + r) * Z_SLOTS + dx + i;
            ra[r][dx] = lbase + slot * 32 + ((h ^ ((slot >> 3) & 1)) << 4);
            asm volatile("" : "+v"(ra[r][dx]));
        }
    // the bias in accumulator layout (register r <-> output channel (r & 3) + 8 * (r >> 2) + 4 * h) lives in LDS, 16 bytes
    // per lane and register group: a drained accumulator set is re-initialised from there by four ds_read_b128 per M tile,
    // dealt out over fragment slots (no VALU; as the C operand of a first MFMA it would cost 16 arch VGPRs the kernel
    // does not have)
    unsigned bsc = lbase + Z_BIAS + lane * 16;
    asm volatile("" : "+v"(bsc));
    {
        u32x4 bq[4];
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
            float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (bias) b4 = *reinterpret_cast<const float4 *>(bias + tg.koff + 8 * rg + 4 * h);
            bq[rg] = u32x4{__float_as_uint(b4.x), __float_as_uint(b4.y), __float_as_uint(b4.z), __float_as_uint(b4.w)};
        }
        if (wave == 0) {
#pragma unroll
            for (int rg = 0; rg < 4; rg++) *(lds_u4 *)(bsc + rg * 1024) = bq[rg];
        }
    }
    // output transposition through the wave's 4-KB scratch: lane (i, h) holds, per M tile m and register group rg, the 4
    // channels 8 rg + 4 h .. +3 of voxel i (8 bytes packed) -> scratch [m][voxel][64 B] with the 16-byte units XORed by
    // (voxel >> 1) & 3 (ds_write_b64, 2-way conflicts: 8 LDS cycles against 6 of transfer); read back as lane L = 16-byte
    // chunk L & 3 of voxel 16 (q & 1) + L / 4 of row q >> 1 (conflict-free) = 1 KB contiguous in HBM per wave store
    const unsigned scr = lbase + Z_SCR + wave * 4096;
    unsigned wsc[4];
#pragma unroll
    for (int rg = 0; rg < 4; rg++) wsc[rg] = scr + i * 64 + ((rg ^ ((i >> 1) & 3)) << 4) + h * 8;
    unsigned rsc = scr + (lane >> 2) * 64 + (((lane & 3) ^ ((lane >> 3) & 3)) << 4);
    asm volatile("" : "+v"(rsc), "+v"(wsc[0]), "+v"(wsc[1]), "+v"(wsc[2]), "+v"(wsc[3]));
    // byte offset of this lane's chunk inside an output plane for store q (row q >> 1, voxels 16 (q & 1) ..): out of range
    // (dropped by the descriptor's range check) when the voxel lies outside the volume
    unsigned voff[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int oh = y0 + 2 * wave + (q >> 1), ow = x0 + (q & 1) * 16 + (lane >> 2);
        voff[q] = (oh < g.Ho && ow < g.Wo) ? (unsigned)((oh * g.Wy + ow) * 64 + (lane & 3) * 16) : 0xfffffff0u;
    }
    asm volatile("" : "+v"(voff[0]), "+v"(voff[1]), "+v"(voff[2]), "+v"(voff[3]));
    // FUSE: the lane's channel octet is fixed on both paths -- staging part tid & 3 (PRO), store chunk lane & 3 (ST)
    float psc[PRO ? 8 : 1], psh[PRO ? 8 : 1];
    if (PRO) {
        const float *sp = in_scale + (size_t)n_ * 32 + (tid & 3) * 8, *tp = in_shift + (size_t)n_ * 32 + (tid & 3) * 8;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            psc[e] = sp[e];
            psh[e] = tp[e];
        }
    }
    const size_t oplane = (size_t)g.Hy * g.Wy * 64;
    char *ybase = reinterpret_cast<char *>(y1) + (size_t)n_ * g.Dy * oplane;
    const char *abase = reinterpret_cast<const char *>(a1) + (size_t)n_ * g.Di * g.Hi * g.Wi * 64;
    const size_t iplane = (size_t)g.Hi * g.Wi * 64;
    const unsigned iplane32 = (unsigned)iplane, oplane32 = (unsigned)oplane;

    // plane index j <-> input plane z' = zb - 1 + j; planes 0 .. nproc-1 carry MFMAs (when inside the volume), plane
    // nproc only drains the last output plane
    const int nproc = (ze - zb) + 2;
    auto zin = [&](int j) { return zb - 1 + j; };
    auto live = [&](int j) { const int z = zin(j); return j < nproc && z >= 0 && z < g.Di; };  // block-uniform
    u32x4 v[2][Z_XR];  // two planes in flight: plane p is staged in v[p & 1] (loaded three planes ahead of its MFMAs)
    __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(abase), 0, 0, 0x00020000);
    auto set_in_plane = [&](int j) {  // descriptor of input plane zin(j) (uniform); zero records = a plane of zeros
        rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(abase + (size_t)max(zin(j), 0) * iplane), 0,
                                                live(j) ? (int)iplane32 : 0, 0x00020000);
    };
    auto stage_load = [&](int set, int u) { v[set][u] = __builtin_amdgcn_raw_buffer_load_b128(rin, (int)rel[u], 0, 0); };
    // PRO: normalise + activate the staged 8 channels (4 VALU per element + one conversion per pair), zeros for parts
    // outside the (y, x) plane or of a plane that does not exist (`lv`, block-uniform)
    auto prologue = [&](u32x4 q, int u, bool lv) {
        const bool ok = lv && rel[u] != 0xfffffff0u;
        unsigned d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            float lo = __uint_as_float(d[e] << 16), hi = __uint_as_float(d[e] & 0xffff0000u);
            lo = __builtin_fmaf(lo, psc[2 * e], psh[2 * e]);
            hi = __builtin_fmaf(hi, psc[2 * e + 1], psh[2 * e + 1]);
            lo = fmaxf(lo, lo * slope);
            hi = fmaxf(hi, hi * slope);
            d[e] = ok ? cvt_pk_bf16(lo, hi) : 0u;
        }
        return u32x4{d[0], d[1], d[2], d[3]};
    };
    // (fused variants: slot = 64 u + tid / 4, so the swizzle bit (slot >> 3) & 1 does not depend on u and the LDS address of
    // part u is wa[0] + 2048 u -- an immediate; five registers fewer)
    auto stage_write = [&](int set, unsigned imgoff, int u, bool lv = true) {
        const u32x4 q = PRO ? prologue(v[set][u], u, lv) : v[set][u];
        const unsigned a_ = FUSE ? wa[0] + 2048u * u : wa[u];
        if (u < Z_XR - 1 || tid < Z_PARTS - (Z_XR - 1) * 256) *(lds_u4 *)(a_ + imgoff) = q;
    };
    auto load_plane = [&](int set, int j) {
        set_in_plane(j);
#pragma unroll
        for (int u = 0; u < Z_XR; u++) stage_load(set, u);
    };
    auto store_plane = [&](int set, unsigned imgoff, bool lv) {
#pragma unroll
        for (int u = 0; u < Z_XR; u++) stage_write(set, imgoff, u, lv);
    };
    i32x4 af[3];  // ring of three A fragments, fetched two fragments ahead (also across planes)
    // fragment f = (r * 3 + dx) * 2 + ks of plane image IMG
#define MVD_Z_READ_A(IMG, F, BUF)                                                                                    \
    {                                                                                                                \
        const u32x4 q_ = *(lds_u4 *)(ra[(F) / 6][((F) >> 1) % 3] + (IMG) * Z_PLANE + ((F) & 1) * Z_HALF);            \
        af[BUF] = *reinterpret_cast<const i32x4 *>(&q_);                                                             \
    }

    // (Statistics epilogue, FUSE bit 0: NOT in this kernel.  Measured in round 3 on three forms -- 16 running sums in VGPRs,
    // transient sums aliased onto the dead accumulator set with AGPR-pinned totals, private LDS slots updated with
    // ds_add_f32 -- the first two push staged input planes or weight fragments into scratch memory (the kernel runs at
    // 254 + 236 of 512 registers), the third makes the launch seven times slower (1.47 ms: LDS float atomics).  The
    // statistics epilogue lives in k_fwd16y, whose 16x16x32 tiling leaves a lane 4 channels instead of 16.)
    f32x16 S[4][2];  // accumulator ring: output plane zo lives in S[(zo - zb + 1) & 3]
    auto bias_init = [&](f32x16 &acc, int rg) {  // acc[4 rg .. 4 rg + 3] = bias
        const u32x4 q = *(lds_u4 *)(bsc + rg * 1024);
        acc[rg * 4 + 0] = __uint_as_float(q.x); acc[rg * 4 + 1] = __uint_as_float(q.y);
        acc[rg * 4 + 2] = __uint_as_float(q.z); acc[rg * 4 + 3] = __uint_as_float(q.w);
    };
    load_plane(0, 0);
    store_plane(0, 0, live(0));
    load_plane(1, 1);
    load_plane(0, 2);
#pragma unroll
    for (int p = 0; p < 27; p++) asm volatile("" : "+a"(bw[p][0]), "+a"(bw[p][1]));
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 32; q++) bias_init(S[q >> 3][(q >> 2) & 1], q & 3);
    MVD_Z_READ_A(0, 0, 0);
    MVD_Z_READ_A(0, 1, 1);

    // plane j with ring position R = j & 3: input image R, accumulator sets NEW = R (output plane z'+1: first
    // contribution, holds the bias), MID = R-1 (z'), OLD = R-2 (z'-1: complete after this plane), DRAIN = R-3 (z'-2:
    // completed by the previous plane, stored during this one, then reset to the bias: it is the next plane's NEW).
    // ONE branch-free body for every plane: a plane that does not exist (z' = -1 or D at the volume faces, and the
    // drain-only plane after the chunk) is a plane of zeros -- its descriptor has zero records, so the staging loads
    // return zeros without touching memory -- and an output plane that is not the chunk's is a descriptor with zero
    // records, so its stores are dropped.  Ablation (MFMAs only) had shown 38.7 cycles per MFMA
    // against 32.4 for the bare loop: ~60 scalar instructions and five branches evaluating plane flags in one clump at
    // every plane boundary, and an in-order wave issues no MFMA behind them (a second, flag-free copy of the body for
    // the interior planes made the register allocator spill 160 registers).  The price: 3 of the Zc + 3 planes of a chunk
    // carry partly or wholly useless MFMAs.
    auto plane = [&](auto Rc, int j) __attribute__((always_inline)) {
        constexpr int R = decltype(Rc)::value;
        constexpr int NEW = R, MID = (R + 3) & 3, OLD = (R + 2) & 3, DRN = (R + 1) & 3, RN = (R + 1) & 3;
        __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(ybase, 0, 0, 0x00020000);
        const bool lvn = live(j + 1);     // PRO: the plane written to LDS during this plane exists
        auto set_out_plane = [&]() {  // the plane held by DRN
            const int zo = zin(j) - 2;
            const bool st = zo >= zb && zo < ze;
            rout = __builtin_amdgcn_make_buffer_rsrc(ybase + (size_t)max(zo, 0) * oplane, 0, st ? (int)oplane32 : 0, 0x00020000);
        };
        auto set_next_in_plane = [&]() {  // input plane j + 3
            const int z2 = zin(j + 3);
            const bool lv = j + 3 < nproc && z2 >= 0 && z2 < g.Di;
            rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(abase + (size_t)max(z2, 0) * iplane), 0,
                                                    lv ? (int)iplane32 : 0, 0x00020000);
        };
        auto epi_pack = [&](int m, int rg) {  // 2 conversions + 1 ds_write_b64
            u32x2 q;
            q.x = cvt_pk_bf16(S[DRN][m][rg * 4 + 0], S[DRN][m][rg * 4 + 1]);
            q.y = cvt_pk_bf16(S[DRN][m][rg * 4 + 2], S[DRN][m][rg * 4 + 3]);
            *(lds_u2 *)(wsc[rg] + m * 2048) = q;
        };
        u32x4 ob;
        auto epi_read = [&](int q) { ob = *(lds_u4 *)(rsc + q * 1024); };
        auto epi_store = [&](int q) { __builtin_amdgcn_raw_buffer_store_b128(ob, rout, (int)voff[q], 0, 0); };
        constexpr unsigned IMGN = RN * Z_PLANE;
        // everything that is not an MFMA is dealt out over the 24 fragment slots of the plane (an MFMA leaves ~24 issue
        // cycles per 32; a clump in front of the plane is paid in full):
        //   f 1-14  one staging ds_write_b128 (plane j+1, loaded during plane j-2) in six of them
        //   f 1-4   epilogue of the drained set: 4 conversions + 2 ds_write_b64 each;  f 0, 4 the two descriptors
        //   f 3-23  one global load (plane j+3, into the registers just written out) in every fourth
        //   f 6-13  scratch read-back and one 1-KB output store, alternating
        //   f 14-21 one ds_read_b128 of the bias table into the drained set each
        //   f 17-20 barrier (plane j+1 visible), wave w in slot 17 + w;   f 22-23 first fragments of plane j+1
#pragma unroll
        for (int f = 0; f < 24; f++) {
            if (f + 2 < 24) MVD_Z_READ_A(R, f + 2, (f + 2) % 3)
            else MVD_Z_READ_A(RN, f + 2 - 24, (f + 2) % 3)  // behind the barrier below
            // The four waves run the same instruction stream, and one barrier per plane would keep them in lockstep: 24
            // staging loads (and 24 13-cycle LDS store transfers) in one window of the CU's single vector-memory pipe.
            // So wave w takes its barrier one fragment slot later than wave w-1 (slots 17 + w: behind its own last staging
            // write, ahead of its first read of the next image) -- after the first plane the waves run w slots apart --
            // and the staging loads sit in slots = 3 mod 4, the writes in slots = 1, 2 mod 4: no two waves load in the
            // same slot time, and the compiler can still count vmcnt (conditional loads cost it the count).
            constexpr int wslot[6] = {1, 2, 6, 9, 10, 14};
#pragma unroll
            for (int u = 0; u < 6; u++)
                if (f == wslot[u]) stage_write(RN & 1, IMGN, u, lvn);
            if (f == 4) set_out_plane();
            if (f == 0) set_next_in_plane();
            if (f == 1) asm volatile("" : "+v"(S[DRN][0]), "+v"(S[DRN][1]));  // keeps the conversions in their slots
            if (f >= 1 && f <= 4) {
                epi_pack((f - 1) >> 1, ((f - 1) & 1) * 2);
                epi_pack((f - 1) >> 1, ((f - 1) & 1) * 2 + 1);
            }
            if ((f & 3) == 3) stage_load(RN & 1, f >> 2);
            if (f >= 6 && f < 14 && !(f & 1)) epi_read((f - 6) >> 1);
            if (f >= 6 && f < 14 && (f & 1)) epi_store((f - 7) >> 1);
            if (f >= 14 && f < 22) bias_init(S[DRN][(f - 14) >> 2], (f - 14) & 3);  // the next plane's NEW set
            if (f >= 17 && f <= 20) {
                // (this wave's plane writes retired in order before the fragment reads already consumed above)
                if (wave == f - 17) asm volatile("s_barrier" ::: "memory");
            }
            const int r = f / 6, dx = (f >> 1) % 3, ks = f & 1;
#pragma unroll
            for (int m = 0; m < 2; m++) {
                const int dy = r - m;  // input row r is output row m shifted by dy - 1
                if (dy < 0 || dy > 2) continue;
                MVD_MFMA16_ZV(S[NEW][m], bw[0 * 9 + dy * 3 + dx][ks], af[f % 3]);
                MVD_MFMA16_ZV(S[MID][m], bw[1 * 9 + dy * 3 + dx][ks], af[f % 3]);
                MVD_MFMA16_ZV(S[OLD][m], bw[2 * 9 + dy * 3 + dx][ks], af[f % 3]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // an MFMA result needs 12 wait states before anything but an accumulating MFMA reads it
        asm volatile("s_nop 7\n\ts_nop 4" : "+v"(S[OLD][0]), "+v"(S[OLD][1]));
    };
    for (int j = 0; j <= nproc; j += 4) {
        plane(ZIdx<0>(), j);
        if (j + 1 > nproc) break;
        plane(ZIdx<1>(), j + 1);
        if (j + 2 > nproc) break;
        plane(ZIdx<2>(), j + 2);
        if (j + 3 > nproc) break;
        plane(ZIdx<3>(), j + 3);
    }
#undef MVD_Z_READ_A
}

static int num_cus16() {
    static int n = 0;
    if (!n) {
        hipDeviceProp_t p;
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
        if (n <= 0) n = 256;
    }
    return n;
}

// k_fwd16z for its shape class; -1: not this kernel's shape
static int launch_fwd16z(const FwdGeom &g, const unsigned short *a1, const unsigned short *w, const float *bias,
                         unsigned short *y1, unsigned short *y2, hipStream_t s, const Fwd16Fuse *fuse = nullptr,
                         int *stats_tiles_only = nullptr) {
    // 32 reduce channels; 32 produce channels, or 32 + 32 into two tensors (the input gradient of a conv that read two
    // concatenated 32-channel tensors: two independent 32 -> 32 problems on the same dy)
    const bool two_out = g.K1 == 32 && g.K2 == 32 && y2 != nullptr;
    if (g.C1 != 32 || g.C2 != 0 || g.K1 != 32 || (g.K2 != 0 && !two_out) || g.ntaps != 27 || g.T != 27 || g.acc) return -1;
    for (int a = 0; a < 3; a++)
        if (g.sa[a] != 1 || g.so[a] != 1 || g.oo[a] != 0) return -1;
    if (g.Dy != g.Do || g.Hy != g.Ho || g.Wy != g.Wo) return -1;
    // at least four 4x8x8 tiles per CU (the threshold of the tile-walking kernels this one replaced) or it does not pay
    const long nitems = (long)g.N * ((g.Do + 3) / 4) * ((g.Ho + 7) / 8) * ((g.Wo + 7) / 8);
    const long ncu = ((long)num_cus16() / 8) * 8;
    if (nitems < 4 * ncu || nitems > (1L << 30)) return -1;
    if ((long)g.N * g.Di * g.Hi * g.Wi * 32 >= (1L << 31)) return -1;  // 32-bit element offsets inside a tile
    // weight index of the raster tap (dz, dy, dx), offsets -1..1.  The geometry builders (conv.hip) never emit the same
    // offset twice, so 27 taps inside [-1, 1]^3 are the full 3x3x3 set; anything else is left to the generic kernels.
    Fwd16ZTile tz;
    memset(&tz, 0, sizeof(tz));
    for (int p = 0; p < 27; p++) {
        const int dz = p / 9 - 1, dy = (p / 3) % 3 - 1, dx = p % 3 - 1;
        int hit = -1;
        for (int t = 0; t < 27; t++)
            if (g.off[t][0] == dz && g.off[t][1] == dy && g.off[t][2] == dx) hit = t;
        if (hit < 0) return -1;
        tz.wsel[p] = g.wt[hit];
    }
    tz.nty = (g.Ho + 7) / 8;
    tz.ntx = (g.Wo + 31) / 32;
    // z chunks: enough workgroups to fill the chip in whole rounds, chunks of >= 8 planes (2 extra input planes
    // and two partly useful MFMA planes per chunk)
    const long cols = (long)g.N * tz.nty * tz.ntx;
    int best = 1;
    double best_cost = 1e30;
    for (int nz = 1; nz <= (g.Do + 7) / 8; nz++) {
        const int zc = (g.Do + nz - 1) / nz;
        const long wgs = cols * ((g.Do + zc - 1) / zc);
        const double cost = (double)((wgs + ncu - 1) / ncu) * (zc + 2.5);
        if (cost < best_cost - 1e-9) { best_cost = cost; best = nz; }
    }
    tz.zc = (g.Do + best - 1) / best;
    tz.nzc = (g.Do + tz.zc - 1) / tz.zc;
    tz.nitems = (int)(cols * tz.nzc);
    if (stats_tiles_only) {  // query: tiles per sample of the statistics epilogue (none here); 0 = this kernel runs
        *stats_tiles_only = 0;
        return 0;
    }
    const bool want_pro = fuse && fuse->in_scale && fuse->in_shift;
    if (want_pro && two_out) return -1;
    auto kfn = want_pro ? k_fwd16z<2> : k_fwd16z<0>;
    if (fuse && fuse->ntiles) *fuse->ntiles = 0;  // (k_fwd16y has the statistics epilogue)
    static PerDeviceFlag configured_z[2];
    if (!configured_z[want_pro]()) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kfn),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)Z_LDS);
        if (e != hipSuccess) {
            set_error("conv fwd16z: cannot raise the dynamic LDS limit: %s", hipGetErrorString(e));
            return 1;
        }
        configured_z[want_pro]() = true;
    }
    const int per_xcd = (tz.nitems + 7) / 8;
    tz.kp = g.K1 + g.K2;
    for (int q = 0; q < (two_out ? 2 : 1); q++) {
        tz.koff = 32 * q;
        hipLaunchKernelGGL(kfn, dim3((unsigned)(per_xcd * 8)), dim3(256), (size_t)Z_LDS, s, g, tz, a1, w, bias, q ? y2 : y1,
                           (float *)nullptr, want_pro ? fuse->in_scale : nullptr, want_pro ? fuse->in_shift : nullptr,
                           fuse ? fuse->slope : 0.f);
        if (check_launch("conv fwd16z (z-marching bf16 mfma, weights in registers)")) return 1;
    }
    return 0;
}

// returns 0 ok, >0 error, -1 unsupported shape
int fwd_bf16_stats_tiles(const FwdGeom &g) {
    int nt = 0;
    if ((g.C1 + g.C2) % 32 || (g.K1 + g.K2) % 32) return 0;
    if (launch_fwd16y(g, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (num_cus16() / 8) * 8, &nt) == 0)
        return nt;
    const int r = launch_fwd16z(g, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &nt);
    return r == 0 ? nt : 0;
}

int fwd_bf16_prologue_ok(const FwdGeom &g) {  // 1: the shape runs on a kernel with the InstanceNorm input prologue
    int nt = 0;
    if ((g.C1 + g.C2) % 32 || (g.K1 + g.K2) % 32 || (g.K2 != 0)) return 0;
    if ((g.C1 == 32 || g.C1 == 64) && g.C2 == 0 &&  // one producer tensor of 32 or 64 channels (k_fwd16y, one or two chunks)
        launch_fwd16y(g, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (num_cus16() / 8) * 8, &nt) == 0)
        return 1;
    if (g.C1 != 32 || g.C2 != 0) return 0;
    return launch_fwd16z(g, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &nt) == 0 ? 1 : 0;
}

int fwd_bf16(const FwdGeom &g, const unsigned short *a1, const unsigned short *a2, const unsigned short *w,
             const float *bias, unsigned short *y1, unsigned short *y2, void *ws, size_t ws_bytes, hipStream_t s,
             const Fwd16Fuse *fuse) {
    const int C = g.C1 + g.C2, K = g.K1 + g.K2;
    if (fuse && fuse->ntiles) *fuse->ntiles = 0;
    if (g.ntaps < 1 || g.ntaps > 27) return -1;
    if (C % 32 != 0 || g.C1 % 32 != 0 || g.C2 % 32 != 0) return -1;
    if (K % 32 != 0 || g.K1 % 32 != 0 || g.K2 % 32 != 0) return -1;
    if (((uintptr_t)a1 | (uintptr_t)a2 | (uintptr_t)w) & 15) return -1;
    int mn[3] = {127, 127, 127}, mx[3] = {-127, -127, -127};
    for (int t = 0; t < g.ntaps; t++)
        for (int a = 0; a < 3; a++) {
            if (g.off[t][a] < mn[a]) mn[a] = g.off[t][a];
            if (g.off[t][a] > mx[a]) mx[a] = g.off[t][a];
        }
    {
        int r = launch_fwd16y(g, a1, a2, w, bias, y1, y2, s, fuse, (num_cus16() / 8) * 8, nullptr);
        if (r >= 0) return r;
        r = launch_fwd16z(g, a1, w, bias, y1, y2, s, fuse);
        if (r >= 0) return r;
        if (!fuse || (!fuse->in_scale && !fuse->tile_stats)) {
            r = launch_fwd16ys(g, a1, a2, w, bias, y1, y2, s, (num_cus16() / 8) * 8);
            if (r >= 0) return r;
        }
    }
    if (fuse && fuse->in_scale) return -1;  // the generic kernels have no input prologue
    const int NT = (K % 64 == 0) ? 2 : 1;
    auto magic = [](int d, int nmax) -> int {
        int m = (1 << 20) / d + 1;  // 20-bit reciprocal: n < 2048 keeps n*m inside int32
        if (nmax > 2048) return -1;
        for (int n = 0; n < nmax; n++)
            if (((n * m) >> 20) != n / d) return -1;
        return m;
    };
    // 3x3x3 stride-1 layers with K % 64 == 0 and at least one 8x8x8 tile per CU: eight waves on a 512-voxel tile -- the
    // weights of a chunk (the larger stream: 110 KB per 32 channels against a 38 KB halo) are fetched once per 512 voxels
    // instead of once per 256, the halo shrinks from 2.34 to 1.95 bytes per byte used (MVD_FWD16_W8=0: four waves)
    static const int w8 = getenv("MVD_FWD16_W8") ? atoi(getenv("MVD_FWD16_W8")) : 1;
    bool unit3 = g.ntaps == 27;
    for (int a = 0; a < 3; a++) unit3 = unit3 && g.sa[a] == 1 && mn[a] == -1 && mx[a] == 1;
    if (w8 && unit3 && NT == 2 && g.Do >= 8) {
        Fwd16Tile tg;
        memset(&tg, 0, sizeof(tg));
        tg.EH = 10; tg.EW = 10; tg.nslots = 1000;
        for (int a = 0; a < 3; a++) tg.min_off[a] = mn[a];
        tg.magHW = magic(100, 1024);
        tg.magW = magic(10, 100);
        for (int t = 0; t < g.ntaps; t++)
            tg.toff[t] = ((g.off[t][0] - mn[0]) * tg.EH + (g.off[t][1] - mn[1])) * tg.EW + (g.off[t][2] - mn[2]);
        tg.ntd = (g.Do + 7) / 8;
        tg.nth = (g.Ho + 7) / 8;
        tg.ntw = (g.Wo + 7) / 8;
        tg.K = K;
        const long wgs8 = (long)g.N * tg.ntd * tg.nth * tg.ntw * (K / 64);
        // measured (round 2, bench_conv --iters 40): 32^3 x 128..256 channels 0.060 / 0.110 ms against 0.064 / 0.117 with four
        // waves; at 64^3 (>= 1024 workgroups) the two co-resident four-wave workgroups overlap better: 0.161 vs 0.160 forward,
        // 0.150 vs 0.142 input gradient -- so only where a CU gets at most a few tiles
        if (tg.magHW >= 0 && tg.magW >= 0 && wgs8 >= 256 && wgs8 < 1024) {
            // (round 3: eight instead of four taps per weight group -- on the idea that a group's 16 KB of weights arrive from
            // L2 later than its 32 MFMAs per wave retire -- measured no different: 0.070 vs 0.069 ms on 128 -> 128 @32^3, 37 %
            // MFMA-busy either way)
            int r = launch_fwd16<2, 2, 4, 8, 8>(g, tg, a1, a2, w, bias, y1, y2, ws, ws_bytes, s);
            if (r >= 0) return r;
        }
    }
    // (3x3x3 stride 2, tried in round 3: a 2 x 4 x 8 output tile on two waves -- 765 halo slots, two workgroups per CU so that one's
    // halo fetch overlaps the other's MFMAs -- measured SLOWER than the 4 x 4 x 8 tile below: 32 -> 64 @128^3 0.295 vs 0.229 ms,
    // 64 -> 128 @64^3 0.111 vs 0.089.  The time of these launches is the per-tap-group weight staging through LDS with its
    // barriers, not the halo: the fix is a z-marching kernel with register-resident weights and a parity-split LDS image.)
    // tile candidates: 4x8x8 (MT = 2) when its halo fits 640 slots, else 4x4x8
    for (int MT = 2; MT >= 1; MT--) {
        Fwd16Tile tg;
        memset(&tg, 0, sizeof(tg));
        const int T3[3] = {4, 4 * MT, 8};
        int E[3];
        for (int a = 0; a < 3; a++) {
            E[a] = (T3[a] - 1) * g.sa[a] + (mx[a] - mn[a]) + 1;
            tg.min_off[a] = mn[a];
        }
        tg.EH = E[1]; tg.EW = E[2];
        tg.nslots = E[0] * E[1] * E[2];
        const int xr_need = (tg.nslots * 4 + 255) / 256;
        int XR;
        if (MT == 2 && xr_need <= 10) XR = 10;
        else if (MT == 1 && xr_need <= 6) XR = 6;
        else if (MT == 1 && xr_need <= 22) XR = 22;
        else continue;
        tg.magHW = magic(tg.EH * tg.EW, XR * 64);
        tg.magW = magic(tg.EW, tg.EH * tg.EW);
        if (tg.magHW < 0 || tg.magW < 0) continue;
        for (int t = 0; t < g.ntaps; t++)
            tg.toff[t] = ((g.off[t][0] - mn[0]) * tg.EH + (g.off[t][1] - mn[1])) * tg.EW + (g.off[t][2] - mn[2]);
        tg.ntd = (g.Do + 3) / 4;
        tg.nth = (g.Ho + 4 * MT - 1) / (4 * MT);
        tg.ntw = (g.Wo + 7) / 8;
        tg.K = K;
        int r = -1;
#define MVD_L16(NT_, MT_, TG_, XR_) launch_fwd16<NT_, MT_, TG_, XR_>(g, tg, a1, a2, w, bias, y1, y2, ws, ws_bytes, s)
        if (MT == 2) {
            r = NT == 2 ? MVD_L16(2, 2, 3, 10) : MVD_L16(1, 2, 4, 10);
        } else if (XR == 6) {
            r = NT == 2 ? MVD_L16(2, 1, 3, 6) : MVD_L16(1, 1, 4, 6);
        } else {
            r = NT == 2 ? MVD_L16(2, 1, 3, 22) : MVD_L16(1, 1, 4, 22);
        }
#undef MVD_L16
        if (r >= 0) return r;
    }
    return -1;
}

int pack_weight16(const float *w, unsigned short *wf, unsigned short *wb, int K, int C, int T, int transposed,
                  hipStream_t s) {
    long total = (long)K * C * T;
    hipLaunchKernelGGL(k_pack_weight16, dim3(cdiv(total, 256)), dim3(256), 0, s, w, wf, wb, K, C, T, transposed);
    return check_launch("pack_weight16");
}

// Every bf16 weight pack of the network in ONE launch after the optimizer step (26 launches of 5-60 us per step
// otherwise).  Jobs travel in the kernel argument; a workgroup finds its job by a scalar scan over the block ranges.
// Element mapping and rounding are those of k_pack_weight16: bit-identical outputs.
struct Pack16Job {
    const float *w;
    unsigned short *wf, *wb;
    int K, C, T, transposed;
    int Cs;     // reduce channels the source holds (<= C): channels Cs .. C-1 are packed as zeros (the padded input conv)
    unsigned blk_begin;
    int tiled;  // 1: 3x3x3 conv -> one workgroup per 16 k x 16 c tile (through LDS)
};
constexpr int PACK16_MAX_JOBS = 64;
struct Pack16Batch {
    int n;
    Pack16Job j[PACK16_MAX_JOBS];
};

// Tiled jobs (3x3x3 convs, C % 32 == 0 and K % 32 == 0): the workgroup reads its 16 x 16 x 27 block of the torch tensor as
// 16 contiguous 1.7 KB runs into LDS and writes both packed layouts in contiguous 256-byte runs (the element-wise form
// reads with a C*27*4-byte lane stride: 280 us for the 26 weights of the network, 4 x the time of the traffic).
__global__ __launch_bounds__(256) void k_pack16_batch(const Pack16Batch pb) {
    __shared__ float tile[16 * 432];  // [k 16][c 16][t 27]
    int q = 0;
    for (int m = 1; m < pb.n; m++)
        if (blockIdx.x >= pb.j[m].blk_begin) q = m;  // scalar scan (block ranges ascend)
    const Pack16Job &J = pb.j[q];
    const unsigned lb = blockIdx.x - J.blk_begin;
    const int tid = threadIdx.x;
    if (!J.tiled) {
        const long i = (long)lb * 256 + tid;
        const long total = (long)J.K * J.C * J.T;
        if (i >= total) return;
        const int k = (int)(i % J.K);
        const int c = (int)((i / J.K) % J.C);
        const int t = (int)(i / ((long)J.K * J.C));
        const float v = J.transposed ? J.w[((size_t)c * J.K + k) * J.T + t]
                                     : (c < J.Cs ? J.w[((size_t)k * J.Cs + c) * J.T + t] : 0.f);
        const unsigned short b = f2bf(v);
        if (J.wf) J.wf[widx16(J.T, J.K, t, c, k)] = b;
        if (J.wb) J.wb[widx16(J.T, J.C, t, k, c)] = b;
        return;
    }
    const int K = J.K, C = J.C;
    const int nct = C >> 4;
    const int k0 = (int)(lb / (unsigned)nct) * 16, c0 = (int)(lb % (unsigned)nct) * 16;
    for (int idx = tid; idx < 16 * 432; idx += 256) {
        const int r = idx / 432, o = idx - r * 432;
        tile[idx] = J.w[((size_t)(k0 + r) * C + c0) * 27 + o];
    }
    __syncthreads();
    // thread = (8-channel half hh, row 0..15, element e 0..7) of the destination: 256 consecutive bytes per half and tap
    const int hh = tid >> 7, row = (tid >> 3) & 15, e = tid & 7;
    if (J.wf) {  // reduce channel c = c0 + 8 hh + e, produce channel k = k0 + row
        unsigned short *dst = J.wf + widx16(27, K, 0, c0 + 8 * hh + e, k0 + row);
        const float *src = tile + row * 432 + (8 * hh + e) * 27;
        for (int t = 0; t < 27; t++) dst[(size_t)t * 4 * K * 8] = f2bf(src[t]);  // widx16: tap stride = 2 * 2 * K * 8
    }
    if (J.wb) {  // reduce channel k = k0 + 8 hh + e, produce channel c = c0 + row
        unsigned short *dst = J.wb + widx16(27, C, 0, k0 + 8 * hh + e, c0 + row);
        const float *src = tile + (8 * hh + e) * 432 + row * 27;
        for (int t = 0; t < 27; t++) dst[(size_t)t * 4 * C * 8] = f2bf(src[t]);
    }
}

int pack_weights16_batch(int n, const float *const *w, unsigned short *const *wf, unsigned short *const *wb, const int *K,
                         const int *C, const int *T, const int *transposed, const int *Csrc, hipStream_t s) {
    int done = 0;
    while (done < n) {
        Pack16Batch pb;
        memset(&pb, 0, sizeof(pb));
        unsigned blocks = 0;
        int m = 0;
        for (; m < PACK16_MAX_JOBS && done + m < n; m++) {
            const int q = done + m;
            Pack16Job &J = pb.j[m];
            J.w = w[q]; J.wf = wf[q]; J.wb = wb[q];
            J.K = K[q]; J.C = C[q]; J.T = T[q]; J.transposed = transposed[q];
            J.Cs = Csrc ? Csrc[q] : J.C;
            J.blk_begin = blocks;
            J.tiled = (J.T == 27 && !J.transposed && J.K % 32 == 0 && J.C % 32 == 0 && J.Cs == J.C) ? 1 : 0;
            blocks += J.tiled ? (unsigned)((J.K / 16) * (J.C / 16)) : (unsigned)cdiv((long)J.K * J.C * J.T, 256);
        }
        pb.n = m;
        if (blocks > 0) hipLaunchKernelGGL(k_pack16_batch, dim3(blocks), dim3(256), 0, s, pb);
        if (check_launch("pack_weights16_batch")) return 1;
        done += m;
    }
    return 0;
}

}  // namespace mvd
