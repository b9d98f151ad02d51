// ======================================================================================= F(2x2x2, 3x3x3) over D, H and W
// fp32 3x3x3 stride-1 convolution (forward and input gradient) with the Winograd F(2,3) transform along all three axes:
// a 2x2x2 output octet reads a 4x4x4 input patch,
//     V = B^T d B (64 positions), M_p[k] += V_p[c] U_p[c][k] with U = (G x G x G) g, y = A^T M A
// -> 64 channel contractions per 8 outputs = 8 per output, 2/3 of F(2x2,3x3) (12) and 8/27 of the direct form.  The
// coefficients are those of F(2x2,3x3) (1 and 1/2; U in multiples of 1/8): the error stays of the same kind.
//
//   * workgroup = 8 waves on a 4 x 8 x 8 voxel tile = 2 x 4 x 4 = 32 octets = ONE 32-row M tile of
//     v_mfma_f32_32x32x2_f32, x 32 output channels; wave (pzh = w >> 2, a = w & 3) owns the 8 positions (pz, a, b) with
//     pz = 2 pzh + {0, 1}: 8 accumulator tiles = 128 accumulator registers, two waves per SIMD, one workgroup per CU;
//   * the D stage of the input transform runs ONCE, while staging: the 6 halo planes of a 16-channel chunk become the
//     8 D-transformed planes (2 octet layers x 4 positions) of the LDS image [8][10 x 10 slots][16 ch + 4 pad];
//     the H and W stages run on the fly on the operands read from it, exactly as in k_fwd_wino2 (8 ds_read_b128,
//     16 v_pk_* and 16 MFMAs per step), so the VALU cost per MFMA is that of k_fwd_wino2;
//   * the next chunk's halo is loaded into registers (6 float4 per thread) while the current chunk's MFMAs run, so
//     the single LDS image needs no second copy and the global latency hides behind the MFMAs;
//   * U is fetched straight from L2 one step ahead of the MFMAs that use it (scalar base + 32-bit lane offset); every
//     U fragment serves the 32 octets of the workgroup: 16 B/clk/CU, the U traffic of k_fwd_wino2;
//   * output transform: W stage in registers, D stage across the wave pairs (w, w + 4) and H stage across the four
//     position rows through the freed halo buffer, 16 bytes per lane and LDS instruction; stores through one scalar
//     base per output column + a 32-bit lane offset; bias and the optional InstanceNorm statistics in the epilogue.
// Octet i of the M tile: layer j = popcount(i >> 2) & 1, quad row qr = (i >> 2) & 3, quad column qc = i & 3.  With the
// 80-byte slot stride and the even-x-first halo rows (k_fwd_wino2) every ds_read_b128 lane group of 16 lanes then has
// one j and all 16 (qr, qc), i.e. 16 distinct 16-byte bank groups: all operand reads are bank-conflict free.
#include "common.h"
#include "conv_geom.h"
#include "wino_common.h"

namespace mvd {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ void k_pack_wino3(const float *__restrict__ w, float *__restrict__ uf, float *__restrict__ ub, int K, int C) {
    const long total = (long)64 * C * K;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    // idx enumerates (pos, c, k) with k fastest
    const int k = (int)(idx % K);
    const long r = idx / K;
    const int c = (int)(r % C), pos = (int)(r / C);
    pack_wino3_entry(w + ((size_t)k * C + c) * 27, uf, ub, K, C, k, c, pos);
}

int pack_weight_wino3(const float *w, float *uf, float *ub, int K, int C, hipStream_t s) {
    const long total = (long)64 * C * K;
    hipLaunchKernelGGL(k_pack_wino3, dim3(cdiv(total, 256)), dim3(256), 0, s, w, uf, ub, K, C);
    return check_launch("pack_weight_wino3");
}

// MVD_WINO3=0 turns the 3-D engine off (the F(2x2,3x3) engine then takes every Winograd layer)
int wino3_enabled() {
    static int m = -1;
    if (m < 0) m = getenv("MVD_WINO3") ? (atoi(getenv("MVD_WINO3")) != 0) : 1;
    return m;
}

struct Wino3Tile {
    int ntd, nth, ntw, nkb;  // 4 x 8 x 8 tiles along D, H, W; 32-channel output blocks
    int nth4;                // 4-row tiles along H of the statistics layout (mvd_conv_stats_tiles)
    int nitems;
    int K;
    unsigned rkb, rtw, rth, rtd;  // w3_recip of nkb, ntw, nth, ntd: the item decomposition stays on the scalar unit
};

// n / d for n * d < 2^31 as a multiply by m = ceil(2^31 / d) and a shift: with e = m d - 2^31 < d the quotient is exact
// while n e < 2^31.  On wave-uniform operands this is s_mul_hi_u32 / s_mul_i32 / s_lshr_b64; a 32-bit udiv goes through
// v_rcp_iflag_f32 and about ten vector instructions.
inline unsigned w3_recip(int d) { return (unsigned)(((1ul << 31) + (unsigned long)d - 1) / (unsigned long)d); }
__device__ __forceinline__ unsigned w3_div(unsigned n, unsigned m) { return (unsigned)(((unsigned long long)n * m) >> 31); }

constexpr int W3S = 20;                    // floats per slot (16 channels + 4 pad: 80-byte stride)
constexpr int W3E = 10;                    // halo extent along H and W
constexpr int W3P = W3E * W3E;             // slots per plane
constexpr int W3IMG = 8 * W3P * W3S;       // the D-transformed image: 16000 floats
constexpr int W3XCH = 4 * 4 * 1024;        // output-transform exchange: 4 position rows x 4 tiles x 64 lanes x 16
constexpr int W3ST = (W3IMG > W3XCH ? W3IMG : W3XCH);  // statistics scratch behind both
constexpr size_t W3LDS = (size_t)(W3ST + 8 * 2 * 64) * sizeof(float);

__global__ __launch_bounds__(512, 1) void k_fwd_wino3(const FwdGeom g, const Wino3Tile tg, const float *__restrict__ a1,
                                                      const float *__restrict__ a2, const float *__restrict__ u,
                                                      const float *__restrict__ bias, float *__restrict__ y1,
                                                      float *__restrict__ y2, float *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float Xs[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int per_xcd = (tg.nitems + 7) >> 3;
    const int item = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if (item >= tg.nitems) return;  // whole workgroup
    // item -> (kb, tw, th, td, n), kb fastest: scalar arithmetic only (host reciprocals, w3_div)
    unsigned r_ = (unsigned)item, q_;
    q_ = w3_div(r_, tg.rkb); const int kb = (int)(r_ - q_ * (unsigned)tg.nkb); r_ = q_;
    q_ = w3_div(r_, tg.rtw); const int tw_ = (int)(r_ - q_ * (unsigned)tg.ntw); r_ = q_;
    q_ = w3_div(r_, tg.rth); const int th_ = (int)(r_ - q_ * (unsigned)tg.nth); r_ = q_;
    q_ = w3_div(r_, tg.rtd); const int td_ = (int)(r_ - q_ * (unsigned)tg.ntd);
    const int n = (int)q_;

    const int C = g.C1 + g.C2;
    const int nch = C >> 4;
    const int od0 = td_ * 4, oh0 = th_ * 8, ow0 = tw_ * 8;
    const int iz0 = od0 - 1, iy0 = oh0 - 1, ix0 = ow0 - 1;

    // position row a and D-position pair pzh of this wave; R = P[ra] + sg * P[rb] (the H stage, as k_fwd_wino2)
    const int a = wave & 3, pzh = wave >> 2;
    const int ra = a == 0 ? 0 : (a == 2 ? 2 : 1);
    const int rb = a == 0 ? 2 : (a == 1 ? 2 : (a == 2 ? 1 : 3));
    const float sg = a == 1 ? 1.f : -1.f;
    const v2f sg2 = {sg, sg};
    // octet of lane i (header): D-transformed plane jo*4 + pz, halo rows 2 qr + {0..3}, patch columns at qc + w2_coff
    const int jo = __builtin_popcount(i >> 2) & 1, qr = (i >> 2) & 3, qc = i & 3;
    const int sbase = (jo * 4 + 2 * pzh) * W3P + 2 * qr * W3E + qc;
    const v4f *xa4 = reinterpret_cast<const v4f *>(Xs + (size_t)(sbase + ra * W3E) * W3S + h * 8);
    const v4f *xb4 = reinterpret_cast<const v4f *>(Xs + (size_t)(sbase + rb * W3E) * W3S + h * 8);
    // weights: step s = (pzl, e) of chunk cc -> block ((cc*4 + 2 pzh + pzl)*4 + a)*2 + e of 4 quarters (b) x [h][k][4]
    const unsigned uq = 2u * tg.K * 4;  // floats between the b quarters
    const unsigned ublk = 4 * uq;       // floats per block
    const unsigned ulane = ((unsigned)(h * tg.K + kb * 32 + i)) << 4;  // BYTES
    const float *uwave = u + (size_t)(16 * pzh + 2 * a) * ublk;

    // staging: thread t < 400 owns slot t >> 2 (row sy, column sx of the 10 x 10 halo) and channel quad t & 3 of all
    // six halo planes; it writes that quad of the eight D-transformed planes
    const bool st_act = tid < 400;
    const int sslot = tid >> 2, squad = tid & 3;
    const int sy = (sslot * 205) >> 11, sx = sslot - sy * W3E;  // sslot / 10 (exact for sslot < 1029)
    const int ih = iy0 + sy, iw = ix0 + sx;
    const bool okyx = st_act && ih >= 0 && ih < g.Hi && iw >= 0 && iw < g.Wi;
    v4f *lds_st = reinterpret_cast<v4f *>(Xs + (size_t)(sy * W3E + (sx >> 1) + 5 * (sx & 1)) * W3S + squad * 4);

    v4f hv[6];  // the raw halo of the next chunk: loaded while the current chunk's MFMAs run
    auto load_halo = [&](int cc) {
        const int c0 = cc * 16;
        const float *src;
        int Cs, cofs;
        if (c0 < g.C1) {
            src = a1; Cs = g.C1; cofs = c0;
        } else {
            src = a2; Cs = g.C2; cofs = c0 - g.C1;
        }
        // byte offset inside a (n, z) plane; only used when okyx (host checks Hi * Wi * Cs * 4 < 2^31)
        const unsigned off = (unsigned)((ih * g.Wi + iw) * Cs + cofs + squad * 4) << 2;
#pragma unroll
        for (int z = 0; z < 6; z++) {
            const int id = iz0 + z;  // wave-uniform
            const float *plane = src + ((size_t)n * g.Di + id) * g.Hi * g.Wi * Cs;
            hv[z] = v4f{0.f, 0.f, 0.f, 0.f};
            if (okyx && id >= 0 && id < g.Di) {
                unsigned o = off;
                asm("" : "+v"(o));  // scalar plane base + 32-bit lane offset
                hv[z] = *reinterpret_cast<const v4f *>(reinterpret_cast<const char *>(plane) + o);
            }
        }
    };

    f32x16 acc[2][4];
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[p][b][r] = 0.f;

    float4 wb[2][4];
#pragma unroll
    for (int b = 0; b < 4; b++)
        wb[0][b] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(uwave + b * uq) + ulane);
    load_halo(0);

    for (int cc = 0; cc < nch; cc++) {
        __syncthreads();  // every wave is done with the previous chunk's image
        if (st_act) {
            // D stage: layer jj reads halo planes 2 jj .. 2 jj + 3: T0 = d0 - d2, T1 = d1 + d2, T2 = d2 - d1, T3 = d1 - d3
#pragma unroll
            for (int jj = 0; jj < 2; jj++) {
                const v4f d0 = hv[2 * jj], d1 = hv[2 * jj + 1], d2 = hv[2 * jj + 2], d3 = hv[2 * jj + 3];
                lds_st[((jj * 4 + 0) * W3P) * (W3S / 4)] = d0 - d2;
                lds_st[((jj * 4 + 1) * W3P) * (W3S / 4)] = d1 + d2;
                lds_st[((jj * 4 + 2) * W3P) * (W3S / 4)] = d2 - d1;
                lds_st[((jj * 4 + 3) * W3P) * (W3S / 4)] = d1 - d3;
            }
        }
        __syncthreads();
        if (cc + 1 < nch) load_halo(cc + 1);
        const float *uc = uwave + (size_t)cc * 32 * ublk;
        // 4 steps (D position pzl, channel quarter e); patch of step s + 1 read before the MFMAs of step s (k_fwd_wino2)
        v4f pa[2][4], pb[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            pa[0][c] = xa4[w2_coff(c) * (W3S / 4)];
            pb[c] = xb4[w2_coff(c) * (W3S / 4)];
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int pzl = s >> 1;
            {   // next step's weights; the chunk's last step fetches step 0 of the next chunk (re-reads its own at the end)
                const float *un = s < 3 ? uc + (size_t)((s + 1) >> 1) * 8 * ublk + (size_t)((s + 1) & 1) * ublk
                                        : (cc + 1 < nch ? uc + (size_t)32 * ublk : uc + (size_t)9 * ublk);
                unsigned ul = ulane;
                asm("" : "+v"(ul));
#pragma unroll
                for (int b = 0; b < 4; b++)
                    wb[(s + 1) & 1][b] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(un + b * uq) + ul);
            }
            const int pn = ((s + 1) >> 1) * W3P * (W3S / 4) + ((s + 1) & 1);  // float4 offset of the next step's patch
            if (s < 3) {
#pragma unroll
                for (int c = 0; c < 4; c++) pa[(s + 1) & 1][c] = xa4[pn + w2_coff(c) * (W3S / 4)];
            }
            __builtin_amdgcn_sched_barrier(0);
            v2f Vl[4], Vh[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                Vl[c] = pa[s & 1][c].xy;
                Vh[c] = pa[s & 1][c].zw;
            }
            Vl[1] = wino2_input_transform(sg2, Vl[0], Vl[1], Vl[2], Vl[3], pb[0].xy, pb[1].xy, pb[2].xy, pb[3].xy);
            Vh[1] = wino2_input_transform(sg2, Vh[0], Vh[1], Vh[2], Vh[3], pb[0].zw, pb[1].zw, pb[2].zw, pb[3].zw);
            __builtin_amdgcn_sched_barrier(0);
            if (s < 3) {
#pragma unroll
                for (int c = 0; c < 4; c++) pb[c] = xb4[pn + w2_coff(c) * (W3S / 4)];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int b = 0; b < 4; b++) acc[pzl][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vl[b].x, wb[s & 1][b].x, acc[pzl][b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < 4; b++) acc[pzl][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vl[b].y, wb[s & 1][b].y, acc[pzl][b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < 4; b++) acc[pzl][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vh[b].x, wb[s & 1][b].z, acc[pzl][b], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < 4; b++) acc[pzl][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vh[b].y, wb[s & 1][b].w, acc[pzl][b], 0, 0, 0);
        }
    }
    const int k = kb * 32 + i;
    const float bv = settled(bias ? bias[k] : 0.f);
    // output transform, W stage in registers: t[pzl][ox] (ox = 0: M0 + M1 + M2, ox = 1: M1 - M2 - M3 over b)
    f32x16 t[2][2];
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            t[p][0][r] = (acc[p][0][r] + acc[p][1][r]) + acc[p][2][r];
            t[p][1][r] = (acc[p][1][r] - acc[p][2][r]) - acc[p][3][r];
        }
    // D stage across the wave pair (a, a + 4): z0 = (M0 + M1) + M2, z1 = M1 - (M2 + M3) over pz.  Exchange layout: a
    // tile of 16 accumulator rows x 64 lanes is [r >> 2][lane][r & 3], so every access is one ds_write_b128 /
    // ds_read_b128 of 16 contiguous bytes per lane (conflict free), and every reader reads the lane index it or its
    // partner wrote.
    __syncthreads();  // all MFMA operand reads of the image are done
    v4f *xr = reinterpret_cast<v4f *>(Xs + (size_t)a * 4096) + lane;  // region of position row a: 4 tiles [oz][ox]
    if (pzh == 1) {
#pragma unroll
        for (int ox = 0; ox < 2; ox++)
#pragma unroll
            for (int rq = 0; rq < 4; rq++) {
                v4f m2, m23;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    m2[e] = t[0][ox][rq * 4 + e];                           // M2
                    m23[e] = t[0][ox][rq * 4 + e] + t[1][ox][rq * 4 + e];  // M2 + M3
                }
                xr[(0 * 2 + ox) * 256 + rq * 64] = m2;
                xr[(1 * 2 + ox) * 256 + rq * 64] = m23;
            }
    }
    __syncthreads();
    if (pzh == 0) {
        // (each wave reads and then rewrites only its own region: no barrier between the two)
#pragma unroll
        for (int ox = 0; ox < 2; ox++)
#pragma unroll
            for (int rq = 0; rq < 4; rq++) {
                const v4f m2 = xr[(0 * 2 + ox) * 256 + rq * 64], m23 = xr[(1 * 2 + ox) * 256 + rq * 64];
                v4f z0, z1;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    z0[e] = (t[0][ox][rq * 4 + e] + t[1][ox][rq * 4 + e]) + m2[e];
                    z1[e] = t[1][ox][rq * 4 + e] - m23[e];
                }
                xr[(0 * 2 + ox) * 256 + rq * 64] = z0;
                xr[(1 * 2 + ox) * 256 + rq * 64] = z1;
            }
    }
    __syncthreads();
    // H stage: wave (oz, oy, ox) = (w >> 2, (w >> 1) & 1, w & 1) finishes output (oz, oy, ox) of every octet from tile
    // [oz][ox] of position rows {0,1,2} (oy = 0: sum) or {1,2,3} (oy = 1: T1 - T2 - T3)
    const int oz = wave >> 2, oy = (wave >> 1) & 1, ox = wave & 1;
    const v4f *xt = reinterpret_cast<const v4f *>(Xs + (size_t)(oz * 2 + ox) * 1024) + lane;
    float vals[16];
#pragma unroll
    for (int rq = 0; rq < 4; rq++) {
        const v4f ta = xt[(oy + 0) * 1024 + rq * 64], tb = xt[(oy + 1) * 1024 + rq * 64], tc = xt[(oy + 2) * 1024 + rq * 64];
#pragma unroll
        for (int e = 0; e < 4; e++)
            vals[rq * 4 + e] = (oy == 0 ? (ta[e] + tb[e]) + tc[e] : (ta[e] - tb[e]) - tc[e]) + bv;
    }
    __builtin_amdgcn_sched_barrier(0);
    // accumulator row r of lane half h is octet m = (r & 3) + 8 (r >> 2) + 4 h: qc = r & 3, m >> 2 = 2 (r >> 2) + h.
    // Addresses: one scalar base per output column (r & 3) + a 32-bit lane offset per row group (r >> 2), as load_halo
    // (the host checks that the offsets fit).  K1 is a multiple of 32, so the whole block writes one of the two tensors.
    const bool two = kb * 32 >= g.K1;  // block-uniform
    const int Ks = two ? g.K2 : g.K1;
    float *ywave = (two ? y2 + (kb * 32 - g.K1) : y1 + kb * 32) +
                   ((((size_t)n * g.Dy + (od0 + oz)) * g.Hy + (oh0 + oy)) * g.Wy + (ow0 + ox)) * Ks;
    unsigned yoff[4];  // BYTES from ywave of column 0, row group r >> 2
    bool yok[4];
#pragma unroll
    for (int rg = 0; rg < 4; rg++) {
        const int m2 = 2 * rg + h;
        const int j = __builtin_popcount(m2) & 1, q = m2 & 3;
        yoff[rg] = (unsigned)(((2 * j * g.Hy + 2 * q) * g.Wy) * Ks + i) << 2;
        yok[rg] = od0 + 2 * j + oz < g.Do && oh0 + 2 * q + oy < g.Ho;
    }
    float ssum[2] = {0.f, 0.f}, ssq[2] = {0.f, 0.f};  // per 4-row half of the tile (the 4x4x8 statistics tiles)
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int ow = ow0 + 2 * (r & 3) + ox;  // wave-uniform
        if (yok[r >> 2] && ow < g.Wo) {
            const float val = vals[r];
            unsigned o = yoff[r >> 2];
            asm("" : "+v"(o));  // scalar column base + 32-bit lane offset
            *reinterpret_cast<float *>(reinterpret_cast<char *>(ywave + (size_t)(2 * (r & 3)) * Ks) + o) = val;
            ssum[(r >> 2) & 1] += val;  // (oh - oh0) >> 2 = q >> 1 = (r >> 2) & 1
            ssq[(r >> 2) & 1] += val * val;
        }
    }
    if (stats != nullptr) {  // block-uniform
        float *st = Xs + W3ST;
#pragma unroll
        for (int sb = 0; sb < 2; sb++) {
            ssum[sb] += __shfl_xor(ssum[sb], 32, 64);
            ssq[sb] += __shfl_xor(ssq[sb], 32, 64);
            if (h == 0) {
                st[((wave * 2 + sb) * 32 + i) * 2 + 0] = ssum[sb];
                st[((wave * 2 + sb) * 32 + i) * 2 + 1] = ssq[sb];
            }
        }
        __syncthreads();
        if (wave < 2 && h == 0) {  // wave sb writes the entry of 4-row tile 2 th_ + sb (when it exists)
            const int sb = wave, th4 = 2 * th_ + sb;
            if (th4 < tg.nth4) {
                float sa = 0.f, sq = 0.f;
#pragma unroll
                for (int w = 0; w < 8; w++) {
                    sa += st[((w * 2 + sb) * 32 + i) * 2 + 0];
                    sq += st[((w * 2 + sb) * 32 + i) * 2 + 1];
                }
                const int tile = (td_ * tg.nth4 + th4) * tg.ntw + tw_;
                float *o = stats + (((size_t)n * (tg.ntd * tg.nth4 * tg.ntw) + tile) * tg.K + k) * 2;
                o[0] = sa;
                o[1] = sq;
            }
        }
    }
}

// The 3-D engine's shape test (plain 3x3x3 stride-1 gather, 32-multiple channels, full stencil in filter or mirrored
// order): -1 when it does not apply.  The caller passes the matching table (uf / ub of mvd_pack_weight_wino3).
int fwd_wino3(const FwdGeom &g, const float *a1, const float *a2, const float *u, const float *bias, float *y1, float *y2,
              hipStream_t s, float *stats, int *stats_done) {
    if (stats_done) *stats_done = 0;
    const int C = g.C1 + g.C2, K = g.K1 + g.K2;
    if (!u || g.ntaps != 27 || g.T != 27) return -1;
    if (C % 32 || g.C1 % 32 || g.C2 % 32 || K % 32 || g.K1 % 32 || g.K2 % 32) return -1;
    for (int ax = 0; ax < 3; ax++)
        if (g.sa[ax] != 1 || g.so[ax] != 1 || g.oo[ax] != 0) return -1;
    if (g.Dy != g.Do || g.Hy != g.Ho || g.Wy != g.Wo) return -1;
    if (((uintptr_t)a1 | (uintptr_t)a2 | (uintptr_t)u) & 15) return -1;
    if ((long)g.Hi * g.Wi * (C > 0 ? (g.C1 > g.C2 ? g.C1 : g.C2) : 0) * 4 >= (1L << 31)) return -1;
    // the kernel's 32-bit store offsets span two output planes and the tile's rows inside them
    if ((long)(2 * g.Hy + 8) * g.Wy * (g.K1 > g.K2 ? g.K1 : g.K2) * 4 >= (1L << 31)) return -1;
    bool plain = true, mirrored = true;
    for (int t = 0; t < 27; t++) {
        const int oz = g.off[t][0], oy = g.off[t][1], ox = g.off[t][2];
        if (oz < -1 || oz > 1 || oy < -1 || oy > 1 || ox < -1 || ox > 1) return -1;
        const int pos = ((oz + 1) * 3 + (oy + 1)) * 3 + (ox + 1);
        if (g.wt[t] != pos) plain = false;
        if (g.wt[t] != 26 - pos) mirrored = false;
    }
    if (!plain && !mirrored) return -1;
    Wino3Tile tg;
    memset(&tg, 0, sizeof(tg));
    tg.ntd = (g.Do + 3) / 4;
    tg.nth = (g.Ho + 7) / 8;
    tg.ntw = (g.Wo + 7) / 8;
    tg.nth4 = (g.Ho + 3) / 4;
    tg.nkb = K / 32;
    tg.K = K;
    const long nitems = (long)g.N * tg.ntd * tg.nth * tg.ntw * tg.nkb;
    if (nitems > (1L << 30)) return -1;
    tg.nitems = (int)nitems;
    // w3_div is exact while item * divisor < 2^31
    int dmax = tg.nkb;
    for (int d : {tg.ntw, tg.nth, tg.ntd}) dmax = d > dmax ? d : dmax;
    if (nitems * dmax >= (1L << 31)) return -1;
    tg.rkb = w3_recip(tg.nkb);
    tg.rtw = w3_recip(tg.ntw);
    tg.rth = w3_recip(tg.nth);
    tg.rtd = w3_recip(tg.ntd);
    static PerDeviceFlag cfgd;
    if (!cfgd()) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_fwd_wino3), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)W3LDS) != hipSuccess) {
            set_error("conv fwd (winograd 3-D): cannot raise the dynamic LDS limit");
            return 1;
        }
        cfgd() = true;
    }
    const unsigned grid = (unsigned)(((nitems + 7) / 8) * 8);
    float *st = (stats && stats_done && g.K2 == 0) ? stats : nullptr;
    hipLaunchKernelGGL(k_fwd_wino3, dim3(grid), dim3(512), W3LDS, s, g, tg, a1, a2, u, bias, y1, y2, st);
    if (st) *stats_done = 1;
    return check_launch("conv fwd (winograd 3-D)");
}

}  // namespace mvd
