// ================================================================================ F(2x2x2, 3x3x3) weight gradient
// fp32 weight gradient of the plain 3x3x3 stride-1 conv with the transposed Winograd F(2,3) along D, H and W: per
// 2x2x2 dy octet and the 4x4x4 input patch that feeds it,
//     V = (B^T x B^T x B^T) d (64 positions), E = (A x A x A) e,  M_p[c][k] += V_p[c] * E_p[k],
//     dW = (G^T x G^T x G^T) M   (k_wgrad_reduce_wino3, fp64)
// -> 64 rank-1 updates per octet = 8 per voxel, against 12 for F(2x2,3x3) (k_wgrad_wino2w12) and 27 for the direct form.
//
//   * tile = 2 x 8 x 8 dy voxels (a 4 x 10 x 10 input halo) = one layer of 4 x 4 octets, as k_wgrad_wino2w12; the GEMM
//     k index is the octet: lane half h takes octet row 2s + h, so one tile is 8 steps (s = 0..1, quad column 0..3) of
//     v_mfma_f32_32x32x2_f32;
//   * 16 waves (four per SIMD, one workgroup per CU); wave (pz, a) owns the positions (pz, a, 0..3): 4 accumulator
//     tiles = 64 accumulator registers; pz = wave >> 2, a = (wave + pz) & 3, so that the four waves of a SIMD are four
//     different position rows, two pair copies and two single copies;
//   * a split walks its tiles on the scalar unit: one division for its first tile, then the digits of nsplit are added
//     with carries (conv_geom.h: tile_walk_at / tile_walk_advance);
//   * the D stage of the input transform runs once, at staging: the 4 halo planes of a (row, column, 4-channel) entry
//     become the 4 D-transformed planes of the same LDS slots, so the image keeps the 2-D kernel's size and two images
//     (double buffering, one barrier per tile) fit; the H and W stages run on the fly exactly as in k_wgrad_wino2w12
//     (sliding window of patch columns, position row a as a template parameter);
//   * dy stays raw in LDS (its D-transformed image would not fit twice): a wave of pz = 1, 2 reads both dy planes of
//     its quad and adds / subtracts them (pz is a runtime value of the wave, only "one plane or two" is a template
//     parameter: 8 code copies instead of 16);
//   * the minus signs of A (row 3) are not applied: E of a position with pz, a or b = 3 is the negated value, and the
//     reduce flips the sign of those partials back (exact in any precision);
//   * bias gradient: wave (pz = 1, a = 1) of the c-block-0 workgroups sums e(z0) + e(z1) of every quad it fetches (row
//     a = 1 needs the whole quad for E anyway).
// Partials [nsplit][64][C][K] (+ bias rows [nsplit][2][K]); no atomics, the reduce sums the splits in a fixed order.
#include "common.h"
#include "conv_geom.h"

namespace mvd {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v2f __attribute__((ext_vector_type(2)));

// (Wg3Tile: conv_geom.h)

constexpr int W3_EA = 10, W3_EB = 8;                                          // halo rows / columns of A and of dy
constexpr int W3_ABYTES = 4 * W3_EA * W3_EA * 128, W3_BBYTES = 2 * W3_EB * W3_EB * 128;
constexpr int W3_IMG = W3_ABYTES + W3_BBYTES;                                  // 67 584 bytes; two images

// PAIR: pz = 1 or 2 (E needs both dy planes); otherwise pz = 0 or 3.  A: position row (H stage).
template <bool PAIR, int A>
__device__ __forceinline__ void wgrad_wino3_body(const int pz, const WgradGeom &g, const Wg3Tile &tg,
                                                 const float *__restrict__ a1, const float *__restrict__ a2,
                                                 const float *__restrict__ b, float *__restrict__ partial,
                                                 float *__restrict__ pbias, float *lds) {
    constexpr int RA = A == 0 ? 0 : (A == 2 ? 2 : 1);
    constexpr int RB = A == 0 ? 2 : (A == 1 ? 2 : (A == 2 ? 1 : 3));
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const int cb = blockIdx.y / tg.nkb, kb = blockIdx.y % tg.nkb;
    const int split = blockIdx.x;
    const int C = g.C1 + g.C2, K = g.K;

    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[j][r] = 0.f;

    const int c0 = cb * 32, k0 = kb * 32;
    const float *asrc;
    int Cs, cofs;
    if (c0 < g.C1) {
        asrc = a1; Cs = g.C1; cofs = c0;
    } else {
        asrc = a2; Cs = g.C2; cofs = c0 - g.C1;
    }
    // staging in three phases, so that few registers hold the next tile: A phase ph = 0, 1: thread t owns the
    // half-entry q = t + 1024 ph < 1600 (halo row / column q >> 4, 2-channel part q & 15) in all four planes (4 x b64);
    // dy phase: thread t owns the entry (slot t >> 3, 4-channel part t & 7) of the 2 x 8 x 8 tile (b128)
    const int planeA = g.Hi * g.Wi * Cs;  // plane z of the halo adds z * planeA
    unsigned relA[2];                      // byte offset of the thread's half-entry in plane 0 of the halo, per phase
#pragma unroll
    for (int ph = 0; ph < 2; ph++) {
        const int q = tid + 1024 * ph, slot = q >> 4;
        const int ya = slot / W3_EA, xa = slot - ya * W3_EA;
        relA[ph] = (unsigned)((ya * g.Wi + xa) * Cs + cofs + (q & 15) * 2) * 4u;
    }
    const int relB = (((tid >> 9) * g.Hb + ((tid >> 6) & 7)) * g.Wb + ((tid >> 3) & 7)) * K + k0 + (tid & 7) * 4;

    v2f ra[4];
    float4 rb;
    // pos: (tw, th, td, n) of the tile, kept by the tile walk (scalar unit); past the last tile: tile 0, no records
    auto load_tile = [&](const TileWalk &pos, bool valid) {
        const int n = valid ? pos.n : 0;
        const int z0 = valid ? pos.td * 2 : 0, y0 = valid ? pos.th * 8 : 0, x0 = valid ? pos.tw * 8 : 0;
        // (z0, y0, x0): first dy voxel; the A halo starts one voxel before it
        const bool intA = z0 >= 1 && y0 >= 1 && x0 >= 1 && z0 + 3 <= g.Di && y0 - 1 + W3_EA <= g.Hi && x0 - 1 + W3_EA <= g.Wi;
        const bool intB = z0 + 2 <= g.Db && y0 + W3_EB <= g.Hb && x0 + W3_EB <= g.Wb;
        const float *baseA = asrc + ((((long)n * g.Di + (z0 - 1)) * g.Hi + (y0 - 1)) * g.Wi + (x0 - 1)) * (long)Cs;
        const float *baseB = b + ((((long)n * g.Db + z0) * g.Hb + y0) * g.Wb + x0) * (long)K;
        // raw buffer loads: a lane outside the volume passes an out-of-range offset and reads zeros; past the last
        // tile the descriptors have no records at all
        const __amdgpu_buffer_rsrc_t rA =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(baseA), 0, valid ? 0x7fffffff : 0, 0x00020000);
        const __amdgpu_buffer_rsrc_t rB =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(baseB), 0, valid ? 0x7fffffff : 0, 0x00020000);
        int pl4 = planeA * 4;
        asm volatile("" : "+s"(pl4));
        struct Ld {
            __amdgpu_buffer_rsrc_t rA, rB;
            bool intA, intB;
            int z0, y0, x0, pl4;
        };
        return Ld{rA, rB, intA, intB, z0, y0, x0, pl4};
    };
    auto issue_a = [&](const auto &L, int ph) {
        const int q = tid + 1024 * ph;
        if (q >= 16 * W3_EA * W3_EA) return;  // store_a skips these threads too
        // one register per phase lives across the tile loop (relA[ph]); the plane offsets are added here (L.pl4 is
        // opaque to the optimiser, which would otherwise hold all eight sums), and the halo coordinates of a tile
        // that crosses the volume's border are recomputed from the thread index in that branch only
        bool inhw = true;  // the thread's halo row and column lie inside the volume
        if (!L.intA) {     // block-uniform; VALU only inside
            int q_ = q;
            asm volatile("" : "+v"(q_));
            const int ya = (q_ >> 4) / W3_EA, xa = (q_ >> 4) - ya * W3_EA;
            const int ih = L.y0 - 1 + ya, iw = L.x0 - 1 + xa;
            inhw = ih >= 0 && ih < g.Hi && iw >= 0 && iw < g.Wi;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            unsigned o = relA[ph] + (unsigned)(u * L.pl4);
            if (!L.intA) {
                const int id = L.z0 - 1 + u;
                o = (inhw && id >= 0 && id < g.Di) ? o : 0xffffffffu;
            }
            ra[u] = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(L.rA, (int)o, 0, 0));
        }
    };
    auto issue_b = [&](const auto &L) {
        unsigned o = (unsigned)relB * 4u;
        if (!L.intB) {
            int t_ = tid;
            asm volatile("" : "+v"(t_));
            const int zb = t_ >> 9, yb = (t_ >> 6) & 7, xb = (t_ >> 3) & 7;
            const int id = L.z0 + zb, ih = L.y0 + yb, iw = L.x0 + xb;
            o = (id < g.Db && ih < g.Hb && iw < g.Wb) ? o : 0xffffffffu;
        }
        rb = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(L.rB, (int)o, 0, 0));
    };
    // D stage of the input transform on the way into LDS: V0 = d0 - d2, V1 = d1 + d2, V2 = d2 - d1, V3 = d1 - d3
    auto store_a = [&](int par, int ph) {
        const int q = tid + 1024 * ph;
        if (q >= 16 * W3_EA * W3_EA) return;
        char *p = reinterpret_cast<char *>(lds) + par * W3_IMG + (q >> 4) * 128 + (q & 15) * 8;
        constexpr int PL = W3_EA * W3_EA * 128;
        *reinterpret_cast<v2f *>(p) = ra[0] - ra[2];
        *reinterpret_cast<v2f *>(p + PL) = ra[1] + ra[2];
        *reinterpret_cast<v2f *>(p + 2 * PL) = ra[2] - ra[1];
        *reinterpret_cast<v2f *>(p + 3 * PL) = ra[1] - ra[3];
    };
    auto store_b = [&](int par) {
        *reinterpret_cast<float4 *>(reinterpret_cast<char *>(lds) + par * W3_IMG + W3_ABYTES + tid * 16) = rb;
    };

    const char *img = reinterpret_cast<const char *>(lds);
    const int abase = pz * (W3_EA * W3_EA * 128) + h * (2 * W3_EA * 128) + i * 4;  // plane pz, octet row h, channel i
    const int bbase = W3_ABYTES + h * (2 * W3_EB * 128) + i * 4;
    const int zoff = pz == 3 ? W3_EB * W3_EB * 128 : 0;  // single-plane waves: pz 0 reads dy plane 0, pz 3 plane 1
    const float esg = pz == 2 ? -1.f : 1.f;              // pair waves: e0 + e1 (pz 1), e0 - e1 (pz 2)
    auto fetch_col = [&](int s, int col, float &pa, float &pb) {
        const int ad = abase + ((4 * s) * W3_EA + col) * 128;
        pa = *reinterpret_cast<const float *>(img + ad + RA * W3_EA * 128);
        pb = *reinterpret_cast<const float *>(img + ad + RB * W3_EA * 128);
    };
    auto rcomb = [&](float pa, float pb) { return A == 1 ? pa + pb : pa - pb; };
    // the dy quad of octet (s, wq) for this wave's pz, before the H and W stages: e0 (z0) / e1 (z1) / e0 +- e1
    auto fetch_e = [&](int s, int wq, float (&e)[4], float (&f)[4]) {
        const int ad = bbase + ((4 * s) * W3_EB + 2 * wq) * 128 + (PAIR ? 0 : zoff);
        e[0] = *reinterpret_cast<const float *>(img + ad);
        e[1] = *reinterpret_cast<const float *>(img + ad + 128);
        e[2] = *reinterpret_cast<const float *>(img + ad + W3_EB * 128);
        e[3] = *reinterpret_cast<const float *>(img + ad + W3_EB * 128 + 128);
        if (PAIR) {
            const int ad1 = ad + W3_EB * W3_EB * 128;
            f[0] = *reinterpret_cast<const float *>(img + ad1);
            f[1] = *reinterpret_cast<const float *>(img + ad1 + 128);
            f[2] = *reinterpret_cast<const float *>(img + ad1 + W3_EB * 128);
            f[3] = *reinterpret_cast<const float *>(img + ad1 + W3_EB * 128 + 128);
        }
    };
    // E row a (row 3 and column 3 un-negated, see above)
    auto make_E = [&](float (&e)[4], const float (&f)[4], float (&E)[4]) {
        if (PAIR) {
#pragma unroll
            for (int q = 0; q < 4; q++) e[q] = fmaf(esg, f[q], e[q]);
        }
        const float f0 = A == 0 ? e[0] : (A == 1 ? e[0] + e[2] : (A == 2 ? e[0] - e[2] : e[2]));
        const float f1 = A == 0 ? e[1] : (A == 1 ? e[1] + e[3] : (A == 2 ? e[1] - e[3] : e[3]));
        E[0] = f0; E[1] = f0 + f1; E[2] = f0 - f1; E[3] = f1;
    };

    float R[4];      // column ring: halo column x lives in slot x & 3
    float V[2][4];   // MFMA A operands, double buffered over the step parity
    float E[2][4];   // MFMA B operands
    const bool bias_wave = PAIR && A == 1 && pz == 1 && pbias != nullptr && cb == 0;  // wave-uniform
    float bsum = 0.f;

    int tile = split;
    int par = 0;
    TileWalk pos = tile_walk_at(split, tg.ntw, tg.nth, tg.ntd);  // the only divisions: once, before the tile loop
    {
        const auto L = load_tile(pos, tile < tg.ntiles);
#pragma unroll
        for (int ph = 0; ph < 2; ph++) {
            issue_a(L, ph);
            store_a(0, ph);
        }
        issue_b(L);
        store_b(0);
        __syncthreads();
    }
    while (tile < tg.ntiles) {
        const int next = tile + tg.nsplit;
        tile_walk_advance(pos, tg.step, tg.ntw, tg.nth, tg.ntd);
        const auto L = load_tile(pos, next < tg.ntiles);
        {   // window of the first octet: columns 0..3 of octet row h, and its dy quad
            float e[4], f[4];
            fetch_e(0, 0, e, f);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                float pa, pb;
                fetch_col(0, c, pa, pb);
                R[c] = rcomb(pa, pb);
            }
            make_E(e, f, E[0]);
            if (PAIR && A == 1 && bias_wave) bsum += (e[0] + e[1]) + (e[2] + e[3]);
            V[0][0] = R[0] - R[2];
            V[0][1] = R[1] + R[2];
            V[0][2] = R[2] - R[1];
            V[0][3] = R[1] - R[3];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const int s = t >> 2, wq = t & 3, cur = t & 1, nxt = cur ^ 1;
            const bool last = t == 7;
            // the next step: (s, wq + 1) needs columns 2wq+4, 2wq+5; after a row's last octet the whole window
            // (columns 0..3) of row s + 1
            const int ns = wq == 3 ? s + 1 : s, nwq = wq == 3 ? 0 : wq + 1;
            float pa[4], pb[4], e[4], f[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(V[cur][j], E[cur][j], acc[j], 0, 0, 0);
                if (!last) {
                    if (j == 0) fetch_e(ns, nwq, e, f);
                    if (wq != 3) {
                        if (j == 1) {
                            fetch_col(ns, 2 * wq + 4, pa[0], pb[0]);
                            fetch_col(ns, 2 * wq + 5, pa[1], pb[1]);
                        }
                    } else if (j == 1 || j == 2) {
                        const int c2 = (j - 1) * 2;
                        fetch_col(ns, c2, pa[c2], pb[c2]);
                        fetch_col(ns, c2 + 1, pa[c2 + 1], pb[c2 + 1]);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (!last) {  // window update + operands of the next step (VALU only; the MFMAs above read V[cur] / E[cur])
                make_E(e, f, E[nxt]);
                if (PAIR && A == 1 && bias_wave) bsum += (e[0] + e[1]) + (e[2] + e[3]);
                if (wq != 3) {
                    R[(2 * wq + 4) & 3] = rcomb(pa[0], pb[0]);
                    R[(2 * wq + 5) & 3] = rcomb(pa[1], pb[1]);
                } else {
#pragma unroll
                    for (int c = 0; c < 4; c++) R[c] = rcomb(pa[c], pb[c]);
                }
                const int x0 = 2 * nwq;
                const float r0 = R[x0 & 3], r1 = R[(x0 + 1) & 3], r2 = R[(x0 + 2) & 3], r3 = R[(x0 + 3) & 3];
                V[nxt][0] = r0 - r2;
                V[nxt][1] = r1 + r2;
                V[nxt][2] = r2 - r1;
                V[nxt][3] = r1 - r3;
            }
            // the next tile rides behind the MFMAs: A phase 0 loaded in step 0 and written (D-transformed) into the
            // other image after step 3, phase 1 loaded then and written after step 6, dy loaded in step 1 and written
            // after step 7.  The other image is free: every wave left it at the previous tile's barrier.
            if (t == 0) issue_a(L, 0);
            if (t == 1) issue_b(L);
            if (t == 3) {
                if (next < tg.ntiles) store_a(par ^ 1, 0);
                issue_a(L, 1);
            }
            if (t == 6 && next < tg.ntiles) store_a(par ^ 1, 1);
            if (t == 7 && next < tg.ntiles) store_b(par ^ 1);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        par ^= 1;
        img = reinterpret_cast<const char *>(lds) + par * W3_IMG;
        tile = next;
    }
    // partial[split][pz][a][b][c][k]; D layout: col = lane & 31 -> k, row -> c
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float *po = partial + ((((size_t)split * 4 + pz) * 4 + A) * 4 + j) * C * K;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            po[(size_t)(c0 + row) * K + k0 + i] = acc[j][r];
        }
    }
    if (bias_wave) pbias[((size_t)split * 2 + h) * K + k0 + i] = bsum;
}

__global__ __launch_bounds__(1024, 1) void k_wgrad_wino3(const WgradGeom g, const Wg3Tile tg, const float *__restrict__ a1,
                                                         const float *__restrict__ a2, const float *__restrict__ b,
                                                         float *__restrict__ partial, float *__restrict__ pbias) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // consecutive waves go to the four SIMDs in turn (measured): rotating the position row by pz gives every
    // SIMD all four rows a, two pair copies and two single copies, instead of the four waves of one row
    const int pz = wave >> 2, a = (wave + pz) & 3;
    // one code copy per (one plane / two planes, position row): every wave runs the same trip counts, so the barriers
    // inside the copies pair up
#define MVD_W3(PAIR, AA) wgrad_wino3_body<PAIR, AA>(pz, g, tg, a1, a2, b, partial, pbias, lds)
    const bool pair = pz == 1 || pz == 2;
    switch (a) {
        case 0: if (pair) MVD_W3(true, 0); else MVD_W3(false, 0); break;
        case 1: if (pair) MVD_W3(true, 1); else MVD_W3(false, 1); break;
        case 2: if (pair) MVD_W3(true, 2); else MVD_W3(false, 2); break;
        default: if (pair) MVD_W3(true, 3); else MVD_W3(false, 3); break;
    }
#undef MVD_W3
}

// dw[k][c][i][j][l] = sum_{pz,a,b} G[pz][i] G[a][j] G[b][l] sgn(pz,a,b) (sum_split M[split][pz][a][b][c][k])
// (fp64, fixed order; sgn = -1 for an odd count of 3s among pz, a, b: the un-negated A rows of k_wgrad_wino3).
// 1024 threads = 64 (c, k) outputs e x 16 position rows (pz, a); each thread sums its four positions b over all splits.
__global__ __launch_bounds__(1024) void k_wgrad_reduce_wino3(const float *__restrict__ partial, float *__restrict__ dw, int C,
                                                             int K, int nsplit) {
    __shared__ double r1[4][4][3][64];  // [pz][a][l][e]: after the W stage
    __shared__ double r2[4][3][3][64];  // [pz][j][l][e]: after the H stage
    const long CK = (long)C * K;
    const long per = 64 * CK;  // one split
    const int e = threadIdx.x & 63, w = threadIdx.x >> 6, pz = w >> 2, a = w & 3;
    const long j = (long)blockIdx.x * 64 + e;
    double m[4] = {0, 0, 0, 0};
    if (j < CK) {
        const float *src = partial + (size_t)w * 4 * CK + j;
        int sp = 0;
        for (; sp + 1 < nsplit; sp += 2) {  // eight loads in flight per thread, added in split order
            float v0[4], v1[4];
#pragma unroll
            for (int bq = 0; bq < 4; bq++) {
                v0[bq] = src[(size_t)sp * per + (size_t)bq * CK];
                v1[bq] = src[(size_t)(sp + 1) * per + (size_t)bq * CK];
            }
#pragma unroll
            for (int bq = 0; bq < 4; bq++) {
                m[bq] += (double)v0[bq];
                m[bq] += (double)v1[bq];
            }
        }
        if (sp < nsplit) {
#pragma unroll
            for (int bq = 0; bq < 4; bq++) m[bq] += (double)src[(size_t)sp * per + (size_t)bq * CK];
        }
    }
    {   // signs, then the W stage: (M G)_l
        const bool neg = (pz == 3) != (a == 3);
        const double m0 = neg ? -m[0] : m[0], m1 = neg ? -m[1] : m[1], m2 = neg ? -m[2] : m[2];
        const double m3 = neg ? m[3] : -m[3];
        r1[pz][a][0][e] = m0 + 0.5 * (m1 + m2);
        r1[pz][a][1][e] = 0.5 * (m1 - m2);
        r1[pz][a][2][e] = 0.5 * (m1 + m2) + m3;
    }
    __syncthreads();
    if (w < 12) {  // H stage: thread (pz', l)
        const int p2 = w / 3, l = w - p2 * 3;
        const double q0 = r1[p2][0][l][e], q1 = r1[p2][1][l][e], q2 = r1[p2][2][l][e], q3 = r1[p2][3][l][e];
        r2[p2][0][l][e] = q0 + 0.5 * (q1 + q2);
        r2[p2][1][l][e] = 0.5 * (q1 - q2);
        r2[p2][2][l][e] = 0.5 * (q1 + q2) + q3;
    }
    __syncthreads();
    if (w >= 9 || j >= CK) return;
    const int jj = w / 3, l = w - jj * 3;  // D stage: thread (j, l) writes the three taps i
    const double q0 = r2[0][jj][l][e], q1 = r2[1][jj][l][e], q2 = r2[2][jj][l][e], q3 = r2[3][jj][l][e];
    const int c = (int)(j / K), k = (int)(j - (long)c * K);
    float *o = dw + ((size_t)k * C + c) * 27 + jj * 3 + l;
    o[0 * 9] = (float)(q0 + 0.5 * (q1 + q2));
    o[1 * 9] = (float)(0.5 * (q1 - q2));
    o[2 * 9] = (float)(0.5 * (q1 + q2) + q3);
}

// MVD_WGRAD_WINO3=0 turns the engine off (k_wgrad_wino2w12 then takes every layer)
int wgrad_wino3_enabled() {
    static int m = -1;
    if (m < 0) m = getenv("MVD_WGRAD_WINO3") ? (atoi(getenv("MVD_WGRAD_WINO3")) != 0) : 1;
    return m;
}

// The engine takes a layer with at least this many work items PER SAMPLE: 2x8x8-voxel tiles x 32x32 channel blocks
// (the length of a split's tile loop is N * items / 256 at one workgroup per CU).  Per sample, so that a data-parallel
// rank runs the engines of the single-process step.  Measured faster than k_wgrad_wino2w12 on every
// stride-1 fp32 layer of the flagship, the smallest being 16^3 x 256 -> 256 = 2048 items (profiles/r05_*); smaller
// layers were not measured and keep F(2x2,3x3).
static const long kWgradWino3MinItemsDefault = 2048;
static long g_wgrad_wino3_min_items =
    getenv("MVD_WGRAD_WINO3_MIN") ? atol(getenv("MVD_WGRAD_WINO3_MIN")) : kWgradWino3MinItemsDefault;
void set_wgrad_wino3_min_items(long n) { g_wgrad_wino3_min_items = n < 0 ? kWgradWino3MinItemsDefault : n; }

bool wgrad_wino3_selected(const WgradGeom &g) {
    if (!wgrad_wino3_enabled() || wino_mode() == 0) return false;
    if (g.ntaps != 27 || g.T != 27 || g.transposed_out || g.C1 % 32 != 0 || g.C2 % 32 != 0 || g.K % 32 != 0) return false;
    if (g.C1 + g.C2 < 32 || g.K < 32) return false;
    for (int a = 0; a < 3; a++)
        if (g.sa[a] != 1 || g.sb[a] != 1) return false;
    for (int t = 0; t < 27; t++)
        if (g.wt[t] != t || g.off[t][0] != t / 9 - 1 || g.off[t][1] != (t / 3) % 3 - 1 || g.off[t][2] != t % 3 - 1 ||
            g.ob[t][0] != 0 || g.ob[t][1] != 0 || g.ob[t][2] != 0)
            return false;
    const long items = (long)((g.Do + 1) / 2) * ((g.Ho + 7) / 8) * ((g.Wo + 7) / 8) * ((g.C1 + g.C2) / 32) * (g.K / 32);
    return items >= g_wgrad_wino3_min_items;
}

static long g_wgrad_wino3_launches = 0;
long wgrad_wino3_launches() { return g_wgrad_wino3_launches; }

size_t wgrad_wino3_ws(int nsplit, int C, int K) { return (size_t)nsplit * ((size_t)64 * C + 2) * K * sizeof(float); }
long wgrad_wino3_min_items() { return g_wgrad_wino3_min_items; }

// false = not run (tile or block count, buffer range, workspace): wgrad_plan goes on to the F(2x2,3x3) kernels
bool wgrad_wino3_plan(const WgradGeom &g, int nsplit, bool want_bias, size_t ws_bytes, WgradPlan *p) {
    const int C = g.C1 + g.C2;
    Wg3Tile tg;
    tg.ntd = (g.Do + 1) / 2;
    tg.nth = (g.Ho + 7) / 8;
    tg.ntw = (g.Wo + 7) / 8;
    const long ntiles = (long)g.N * tg.ntd * tg.nth * tg.ntw;
    if (ntiles > (1L << 30)) return false;
    tg.ntiles = (int)ntiles;
    tg.nkb = g.K / 32;
    const int ncb = C / 32;
    if ((long)ncb * tg.nkb > 65535) return false;
    if (nsplit > ntiles) nsplit = (int)ntiles;
    if (nsplit < 1) nsplit = 1;
    tg.nsplit = nsplit;
    tg.step = tile_walk_at(nsplit, tg.ntw, tg.nth, tg.ntd);
    // the buffer offsets of one tile (plane 3 of the A halo, the far corner of dy) must fit the 31-bit buffer range
    if ((long)4 * g.Hi * g.Wi * g.C1 * 4 >= (1L << 31) || (long)4 * g.Hi * g.Wi * g.C2 * 4 >= (1L << 31) ||
        (long)2 * g.Hb * g.Wb * g.K * 4 >= (1L << 31))
        return false;
    if (wgrad_wino3_ws(nsplit, C, g.K) > ws_bytes) return false;
    p->kernel = WG_WINO3;
    p->reduce = WGR_WINO3;
    p->bias_src = want_bias ? WGB_WINO3 : WGB_NONE;
    p->bias_rows = want_bias ? nsplit * 2 : 0;
    p->bias_off = (size_t)nsplit * 64 * C * g.K * sizeof(float);
    p->TD = 2; p->TH = 8; p->TW = 8;
    p->ntd = tg.ntd; p->nth = tg.nth; p->ntw = tg.ntw;
    p->ntiles = ntiles;
    p->nsplit = nsplit;
    p->partials = 1;
    p->ncb = ncb; p->nkb = tg.nkb;
    p->needed_ws = wgrad_wino3_ws(nsplit, C, g.K);
    p->t3 = tg;
    return true;
}

int wgrad_wino3_launch(const WgradPlan &p, const WgradGeom &g, const float *a1, const float *a2, const float *b, float *dw,
                       void *ws, hipStream_t s, float *dbias, int *dbias_done) {
    const int C = g.C1 + g.C2, nsplit = p.nsplit;
    float *partial = reinterpret_cast<float *>(ws);
    float *pbias = p.bias_rows ? reinterpret_cast<float *>(reinterpret_cast<char *>(ws) + p.bias_off) : nullptr;
    static PerDeviceFlag cfgd;
    if (!cfgd()) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_wgrad_wino3), hipFuncAttributeMaxDynamicSharedMemorySize,
                                2 * W3_IMG) != hipSuccess) {
            set_error("conv wgrad (winograd 3-D): cannot raise the dynamic LDS limit");
            return 1;
        }
        cfgd() = true;
    }
    g_wgrad_last_kernel = WG_WINO3;
    hipLaunchKernelGGL(k_wgrad_wino3, dim3(nsplit, p.ncb * p.nkb), dim3(1024), (size_t)2 * W3_IMG, s, g, p.t3, a1, a2, b,
                       partial, pbias);
    if (check_launch("conv wgrad (winograd 3-D)")) return 1;
    g_wgrad_wino3_launches++;
    if (pbias) {
        if (dbias_reduce(pbias, dbias, g.K, p.bias_rows, s)) return 1;
        *dbias_done = 1;
    }
    hipLaunchKernelGGL(k_wgrad_reduce_wino3, dim3(cdiv((long)C * g.K, 64)), dim3(1024), 0, s, partial, dw, C, g.K, nsplit);
    return check_launch("conv wgrad reduce (winograd 3-D)");
}

}  // namespace mvd
