// fp32 1x3x3 stride-1 convolution (forward and input gradient) with the Winograd F(2x2,3x3) transform over H and W:
// the 9-tap in-plane layers of a 2-D network ([N,C,1,H,W] views) and of anisotropic 3-D plans.
//
// The arithmetic scheme is k_fwd_wino2's (conv_wino.hip): 32 quads x 32 output channels per workgroup, four waves = the
// four position rows of the 4x4 patch, v_mfma_f32_32x32x2f32, packed weights fetched from L2 in the wave-uniform base +
// 32-bit lane offset form, output transform crossed through LDS.  What differs is the tile.  There is ONE depth tap, so
// nothing accumulates across planes and a plane needs no neighbours: the (n, d) planes of the NDHWC tensor are one flat
// axis of P = N * D independent planes, and a workgroup takes FOUR CONSECUTIVE PLANES x 4 x 8 outputs.  That keeps the
// quad -> LDS slot assignment of k_fwd_wino2 (quad i = plane i & 3, column (i >> 2) & 3, quad row i >> 4; even x first in
// a 10-slot row; 144-byte slots), the one for which all eight ds_read_b128 of a step are bank-conflict free, and it
// serves D = 1 (four samples per workgroup) and D > 1 (the anisotropic case) with the same index math.  The halo is
// 4 planes x 6 x 10 slots (no depth halo): 34.5 KB, 1.875 input lines per output voxel instead of the 2.8 of the 3-D tile.
//
// A 32-channel chunk is 4 steps of 16 MFMAs (k_fwd_wino2: 12), so the staging of the next chunk has less to hide behind:
// the global loads of chunk cc + 1 are issued into registers BEFORE the MFMA steps of chunk cc and stored to LDS after
// them (8 float4 per thread); two workgroups share a CU (launch bounds 256 x 2: the staging registers cost the third).
#include "common.h"
#include "conv_geom.h"
#include "wino_common.h"

namespace mvd {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PXS = 36;                          // floats per halo slot (32 + 4 pad)
constexpr int PEH = 6, PEW = 10, PEHW = 60;      // halo of one plane of the tile: 6 x 10 slots
constexpr int PPL = 4;                           // planes per tile
constexpr int PNQ = 2 * PPL;                     // staging passes: 240 threads x three rows of a plane

struct Wino2pTile {
    int P;               // planes = N * D
    int ntp, nth, ntw, nkb;
    int nitems;
    int K;
};

// (table layout u2pidx and the entry arithmetic pack_wino2p_entry: wino_common.h, shared with k_pack_batch)
// w: torch weight [K][C][1][3][3] (= Conv2d [K][C][3][3]).  uf: forward (reduce C, produce K); ub: input gradient (reduce
// K, produce C, filter mirrored in both axes).  One summation order here and in k_pack_batch: bit-identical tables.
__global__ void k_pack_wino2p(const float *__restrict__ w, float *__restrict__ uf, float *__restrict__ ub, int K, int C) {
    const long total = (long)16 * C * K;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int k = (int)(idx % K);
    long r = idx / K;
    const int c = (int)(r % C);
    const int pos = (int)(r / C);
    pack_wino2p_entry(w + ((size_t)k * C + c) * 9, uf, ub, K, C, k, c, pos);
}

int pack_weight_wino2p(const float *w, float *uf, float *ub, int K, int C, hipStream_t s) {
    const long total = (long)16 * C * K;
    hipLaunchKernelGGL(k_pack_wino2p, dim3(cdiv(total, 256)), dim3(256), 0, s, w, uf, ub, K, C);
    return check_launch("pack_weight_wino2p");
}

__global__ __launch_bounds__(256, 2) void k_fwd_wino2p(const FwdGeom g, const Wino2pTile tg, const float *__restrict__ a1,
                                                       const float *__restrict__ a2, const float *__restrict__ u,
                                                       const float *__restrict__ bias, float *__restrict__ y1,
                                                       float *__restrict__ y2) {
    extern __shared__ __attribute__((aligned(16))) float Xs[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int per_xcd = (tg.nitems + 7) >> 3;
    const int item = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (item >= tg.nitems) return;  // whole workgroup
    unsigned r_ = (unsigned)item;
    const int kb = __builtin_amdgcn_readfirstlane((int)(r_ % (unsigned)tg.nkb)); r_ /= (unsigned)tg.nkb;
    const int tw_ = __builtin_amdgcn_readfirstlane((int)(r_ % (unsigned)tg.ntw)); r_ /= (unsigned)tg.ntw;
    const int th_ = __builtin_amdgcn_readfirstlane((int)(r_ % (unsigned)tg.nth));
    const int tp_ = __builtin_amdgcn_readfirstlane((int)(r_ / (unsigned)tg.nth));

    const int C = g.C1 + g.C2;
    const int nch = C >> 5;
    const int p0 = tp_ * PPL, oh0 = th_ * 4, ow0 = tw_ * 8;
    const int iy0 = oh0 - 1, ix0 = ow0 - 1;

    // position row a = wave: R = P[ra] + sg * P[rb]
    const int ra = wave == 0 ? 0 : (wave == 2 ? 2 : 1);
    const int rb = wave == 0 ? 2 : (wave == 1 ? 2 : (wave == 2 ? 1 : 3));
    const float sg = wave == 1 ? 1.f : -1.f;
    const v2f sg2 = {sg, sg};
    const int sbase = ((i & 3) * PEH + 2 * (i >> 4)) * PEW + ((i >> 2) & 3);
    const v4f *xa4 = reinterpret_cast<const v4f *>(Xs + (size_t)(sbase + ra * PEW) * PXS + h * 16);
    const v4f *xb4 = reinterpret_cast<const v4f *>(Xs + (size_t)(sbase + rb * PEW) * PXS + h * 16);
    // weights: step (cc, e) -> block (cc*4 + a)*4 + e of 4 quarters (b) x [h][k][4]
    const unsigned uq = 2u * tg.K * 4;  // floats between the b quarters
    const unsigned ustep = 4 * uq;      // floats between consecutive e steps
    const unsigned ulane = ((unsigned)(h * tg.K + kb * 32 + i)) << 4;  // BYTES
    const float *uwave = u + (size_t)wave * 4 * ustep;

    // halo staging: 240 threads cover three rows of 10 slots x 8 float4 per pass; pass q holds plane q >> 1, rows
    // y = r3 + 3 * (q & 1)
    const bool st_act = tid < 240;
    const int r3 = tid / 80, rem = tid - r3 * 80;
    const int sx = rem >> 3, part = rem & 7;
    const int iw = ix0 + sx, ihA = iy0 + r3, ihB = ihA + 3;
    const bool okw = st_act && iw >= 0 && iw < g.Wi;
    const bool okA = okw && ihA >= 0 && ihA < g.Hi, okB = okw && ihB >= 0 && ihB < g.Hi;
    v4f *lds_st = reinterpret_cast<v4f *>(Xs + (size_t)(r3 * PEW + (sx >> 1) + 5 * (sx & 1)) * PXS + part * 4);

    const int k = kb * 32 + i;
    f32x16 acc[4];
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[b][r] = 0.f;

    v4f v[PNQ];  // the staged chunk in flight
    auto stage_load = [&](int cc) {
        const int c0 = cc * 32;
        const float *src;
        int Cs, cofs;
        if (c0 < g.C1) {
            src = a1; Cs = g.C1; cofs = c0;
        } else {
            src = a2; Cs = g.C2; cofs = c0 - g.C1;
        }
        // byte offsets inside a plane; only used when okA / okB (host checks Hi * Wi * Cs * 4 < 2^31)
        const unsigned offA = (unsigned)((ihA * g.Wi + iw) * Cs + cofs + part * 4) << 2;
        const unsigned offB = offA + ((unsigned)(3 * g.Wi * Cs) << 2);
#pragma unroll
        for (int q = 0; q < PNQ; q++) {
            const int pl = p0 + (q >> 1);  // wave-uniform
            const float *plane = src + (size_t)pl * g.Hi * g.Wi * Cs;
            const bool ok = ((q & 1) ? okB : okA) && pl < tg.P;
            v[q] = v4f{0.f, 0.f, 0.f, 0.f};
            if (ok) {
                unsigned o = (q & 1) ? offB : offA;
                asm("" : "+v"(o));  // scalar plane base + 32-bit lane offset
                v[q] = *reinterpret_cast<const v4f *>(reinterpret_cast<const char *>(plane) + o);
            }
        }
    };
    stage_load(0);

    for (int cc = 0; cc < nch; cc++) {
        const float *uc = uwave + (size_t)cc * 16 * ustep;  // 4 position rows x 4 steps
        float4 wb[2][4];
#pragma unroll
        for (int b = 0; b < 4; b++)
            wb[0][b] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(uc + b * uq) + ulane);
        __syncthreads();  // every wave is done with the previous chunk's halo
#pragma unroll
        for (int q = 0; q < PNQ; q++)
            if (st_act) lds_st[((q >> 1) * PEHW + 3 * (q & 1) * PEW) * (PXS / 4)] = v[q];
        __syncthreads();
        if (cc + 1 < nch) stage_load(cc + 1);  // in flight during this chunk's MFMAs
        v4f pa[2][4], pb[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            pa[0][c] = xa4[w2_coff(c) * (PXS / 4)];
            pb[c] = xb4[w2_coff(c) * (PXS / 4)];
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (e < 3) {  // next step's weights and the P[ra] rows of its patch
                const float *un = uc + (size_t)(e + 1) * ustep;  // wave-uniform
                unsigned ul = ulane;
                asm("" : "+v"(ul));
#pragma unroll
                for (int b = 0; b < 4; b++)
                    wb[(e + 1) & 1][b] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(un + b * uq) + ul);
#pragma unroll
                for (int c = 0; c < 4; c++) pa[(e + 1) & 1][c] = xa4[e + 1 + w2_coff(c) * (PXS / 4)];
            }
            __builtin_amdgcn_sched_barrier(0);
            v2f Vl[4], Vh[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                Vl[c] = pa[e & 1][c].xy;
                Vh[c] = pa[e & 1][c].zw;
            }
            Vl[1] = wino2_input_transform(sg2, Vl[0], Vl[1], Vl[2], Vl[3], pb[0].xy, pb[1].xy, pb[2].xy, pb[3].xy);
            Vh[1] = wino2_input_transform(sg2, Vh[0], Vh[1], Vh[2], Vh[3], pb[0].zw, pb[1].zw, pb[2].zw, pb[3].zw);
            __builtin_amdgcn_sched_barrier(0);
            if (e < 3) {
#pragma unroll
                for (int c = 0; c < 4; c++) pb[c] = xb4[e + 1 + w2_coff(c) * (PXS / 4)];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int b = 0; b < 4; b++) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vl[b].x, wb[e & 1][b].x, acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < 4; b++) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vl[b].y, wb[e & 1][b].y, acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < 4; b++) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vh[b].x, wb[e & 1][b].z, acc[b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < 4; b++) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vh[b].y, wb[e & 1][b].w, acc[b], 0, 0, 0);
        }
    }
    const float bv = settled(bias ? bias[k] : 0.f);
    // output transform.  Column half in registers, row half across the four waves through LDS.
    f32x16 t0, t1;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        t0[r] = (acc[0][r] + acc[1][r]) + acc[2][r];
        t1[r] = (acc[1][r] - acc[2][r]) - acc[3][r];
    }
    __syncthreads();  // all MFMA operand reads of the halo are done
    {
        float *xo = Xs + (size_t)wave * 2048 + lane;  // 4 x 2048 floats <= the 8640 of the halo
#pragma unroll
        for (int r = 0; r < 16; r++) {
            xo[r * 64] = t0[r];
            xo[1024 + r * 64] = t1[r];
        }
    }
    __syncthreads();
    // wave (yr, yc) finishes output voxel (yr, yc) of each quad.  Accumulator row r of lane half h is quad
    // q = (r & 3) + 8 * (r >> 2) + 4 * h = (plane r & 3, column 2 * ((r >> 2) & 1) + h, quad row r >> 3)
    const int yr = wave >> 1, yc = wave & 1;
    const float *xt = Xs + (size_t)yc * 1024 + lane;
    const int owl = ow0 + yc + 2 * h;  // + 4 * ((r >> 2) & 1)
    float vals[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const float ta = xt[(size_t)(yr + 0) * 2048 + r * 64], tb = xt[(size_t)(yr + 1) * 2048 + r * 64],
                    tc = xt[(size_t)(yr + 2) * 2048 + r * 64];
        vals[r] = (yr == 0 ? (ta + tb) + tc : (ta - tb) - tc) + bv;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int pl = p0 + (r & 3), oh = oh0 + 2 * (r >> 3) + yr;  // wave-uniform
        const int ow = owl + 4 * ((r >> 2) & 1);
        if (pl < tg.P && oh < g.Ho && ow < g.Wo) {
            const size_t ov = ((size_t)pl * g.Hy + oh) * g.Wy + ow;  // (n, d) planes are contiguous: Dy == Do == Di
            if (k < g.K1)
                y1[ov * g.K1 + k] = vals[r];
            else
                y2[ov * g.K2 + (k - g.K1)] = vals[r];
        }
    }
}

long wino2p_items(int N, int D, int H, int W, int K) {
    return (long)(((long)N * D + PPL - 1) / PPL) * ((H + 3) / 4) * ((W + 7) / 8) * (K / 32);
}

// returns -1 when the problem is not a plain 1x3x3 stride-1 gather with 32-multiple channels (caller falls back)
int fwd_wino2p(const FwdGeom &g, const float *a1, const float *a2, const float *u, const float *bias, float *y1, float *y2,
               hipStream_t s) {
    const int C = g.C1 + g.C2, K = g.K1 + g.K2;
    if (!u || g.ntaps != 9 || g.T != 9 || g.acc) return -1;
    if (C % 32 || g.C1 % 32 || g.C2 % 32 || K % 32 || g.K1 % 32 || g.K2 % 32 || g.C1 <= 0 || g.K1 <= 0) return -1;
    for (int a = 0; a < 3; a++)
        if (g.sa[a] != 1 || g.so[a] != 1 || g.oo[a] != 0) return -1;
    if (g.Dy != g.Do || g.Hy != g.Ho || g.Wy != g.Wo) return -1;
    if (g.Di != g.Do || g.Hi != g.Ho || g.Wi != g.Wo) return -1;  // the plane index of the input is that of the output
    if (((uintptr_t)a1 | (uintptr_t)a2 | (uintptr_t)u) & 15) return -1;
    if ((g.C2 && !a2) || (g.K2 && !y2)) return -1;
    // the 9 taps must be the full 1x3x3 stencil, in filter order (forward) or mirrored (input gradient); the caller
    // passes the matching table (uf / ub of mvd_pack_weight_wino2p).  (3,3,1) and (3,1,3) kernels fail here.
    bool plain = true, mirrored = true;
    for (int t = 0; t < 9; t++) {
        const int oz = g.off[t][0], oy = g.off[t][1], ox = g.off[t][2];
        if (oz != 0 || oy < -1 || oy > 1 || ox < -1 || ox > 1) return -1;
        const int pos = (oy + 1) * 3 + (ox + 1);
        if (g.wt[t] != pos) plain = false;
        if (g.wt[t] != 8 - pos) mirrored = false;
    }
    if (!plain && !mirrored) return -1;
    const int cmax = g.C1 > g.C2 ? g.C1 : g.C2;
    if ((long)g.Hi * g.Wi * cmax * 4 >= (1L << 31)) return -1;  // 32-bit byte offsets inside a plane
    if ((long)K * 32 >= (1L << 27)) return -1;                  // 32-bit weight lane offset
    const long P = (long)g.N * g.Di;
    Wino2pTile tg;
    memset(&tg, 0, sizeof(tg));
    tg.ntp = (int)((P + PPL - 1) / PPL);
    tg.nth = (g.Ho + 3) / 4;
    tg.ntw = (g.Wo + 7) / 8;
    tg.nkb = K / 32;
    tg.K = K;
    const long nitems = (long)tg.ntp * tg.nth * tg.ntw * tg.nkb;
    if (P > (1L << 30) || nitems > (1L << 30)) return -1;
    tg.P = (int)P;
    tg.nitems = (int)nitems;
    const size_t lds = (size_t)PPL * PEHW * PXS * sizeof(float);
    const unsigned grid = (unsigned)(((nitems + 7) / 8) * 8);
    hipLaunchKernelGGL(k_fwd_wino2p, dim3(grid), dim3(256), lds, s, g, tg, a1, a2, u, bias, y1, y2);
    return check_launch("conv fwd (winograd 2-D, 9 taps)");
}

}  // namespace mvd
