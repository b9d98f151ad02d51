// Shared pieces of the fp32 Winograd forward-type kernels (conv_wino.hip: k_fwd_wino2, conv_wino3.hip: k_fwd_wino3).
#pragma once
#include "common.h"

namespace mvd {

// Packed fp32 VALU through inline asm.  On gfx950 every fp32 VALU instruction takes ~3 cycles away from the fp32 MFMA
// pipe of its SIMD (tools/probes/valu_mix_probe.hip: they do not overlap, not even across waves), so the input transform
// is written with v_pk_fma_f32 / v_pk_add_f32 on the register pairs ds_read_b128 delivers -- 16 instead of 32 VALU
// instructions per 16 MFMAs.  Plain <2 x float> arithmetic does not survive: the backend's pre-emit peephole unpacks
// packed F32 instructions it finds behind an MFMA.
// HAZARD: a VALU write needs 2 wait states before an MFMA reads the register as SrcA/B, and the compiler's hazard
// recognizer does not look inside inline asm -- hence the trailing s_nop 1 of every block whose results feed MFMAs.
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

// One half (two of the four channels of a float4) of the F(2x2,3x3) input transform of a step:
//   R_c = a_c + sg * b_c (c = 0..3: the four patch columns);  V0 = R0 - R2, V1 = R1 + R2, V2 = R2 - R1, V3 = R1 - R3
// in place: a0 -> V0, a2 -> V2, a3 -> V3; V1 is returned (a1 is consumed as scratch for R1).
__device__ __forceinline__ v2f wino2_input_transform(v2f sg, v2f &a0, v2f a1, v2f &a2, v2f &a3, v2f b0, v2f b1, v2f b2,
                                                     v2f b3) {
    v2f t;
    asm("v_pk_fma_f32 %0, %5, %6, %0\n\t"
        "v_pk_fma_f32 %1, %5, %7, %1\n\t"
        "v_pk_fma_f32 %2, %5, %8, %2\n\t"
        "v_pk_fma_f32 %3, %5, %9, %3\n\t"
        "v_pk_add_f32 %0, %0, %2 neg_lo:[0,1] neg_hi:[0,1]\n\t"  // V0 = R0 - R2
        "v_pk_add_f32 %3, %1, %3 neg_lo:[0,1] neg_hi:[0,1]\n\t"  // V3 = R1 - R3
        "v_pk_add_f32 %4, %1, %2\n\t"                            // V1 = R1 + R2
        "v_pk_add_f32 %2, %2, %1 neg_lo:[0,1] neg_hi:[0,1]\n\t"  // V2 = R2 - R1
        "s_nop 1"
        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "=&v"(t)
        : "v"(sg), "v"(b0), "v"(b1), "v"(b2), "v"(b3));
    return t;
}

// slot offset of patch column c (0..3) from a quad's origin in a 10-slot halo row that stores the even x first
// (x -> (x >> 1) + 5 * (x & 1)): 0, 5, 1, 6
__device__ __forceinline__ constexpr int w2_coff(int c) { return (c >> 1) + 5 * (c & 1); }

// ---------------------------------------------------------------------------- F(2x2,3x3) tables of 1x3x3 layers (conv_wino2p.hip)
// U layout: [cc][a][e4][b][h][k][4], reduce channel c = cc*32 + h*16 + e4*4 + c4 (u2idx of conv_wino.hip without gz)
__host__ __device__ inline size_t u2pidx(int K, int cc, int a, int b, int h, int k, int e) {
    return (((((((size_t)cc * 4 + a) * 4 + (e >> 2)) * 4 + b) * 2 + h) * K + k) << 2) + (e & 3);
}

// one (a, b, c, k) entry of uf (forward: reduce C, produce K) and ub (input gradient: reduce K, produce C, filter mirrored
// in both axes) from the 9 taps wp[i*3 + j] of the (k, c) pair; pos = a*4 + b.  One summation order for the per-layer and
// the batched pack: bit-identical tables.
__device__ __forceinline__ void pack_wino2p_entry(const float *wp, float *__restrict__ uf, float *__restrict__ ub, int K,
                                                  int C, int k, int c, int pos) {
    const float G[4][3] = {{1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.f, 0.f, 1.f}};
    const int b = pos & 3, a = (pos >> 2) & 3;
    if (uf) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) s += G[a][i] * G[b][j] * wp[i * 3 + j];
        uf[u2pidx(K, c >> 5, a, b, (c >> 4) & 1, k, c & 15)] = s;
    }
    if (ub) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) s += G[a][i] * G[b][j] * wp[(2 - i) * 3 + (2 - j)];
        ub[u2pidx(C, k >> 5, a, b, (k >> 4) & 1, c, k & 15)] = s;
    }
}

// ---------------------------------------------------------------------------- F(2x2x2,3x3x3) weight tables (conv_wino3.hip)
// U3 layout: [cc][pz][a][e][b][h][k][4], reduce channel c = cc*16 + h*8 + e*4 + c4 (e: 4-channel step of the chunk)
__host__ __device__ inline size_t u3idx(int K, int cc, int pz, int a, int b, int h, int k, int e8) {
    return ((((((((size_t)cc * 4 + pz) * 4 + a) * 2 + (e8 >> 2)) * 4 + b) * 2 + h) * K + k) << 2) + (e8 & 3);
}

// U_{pz,a,b} of one (k, c) pair from its 27 taps wp[(i*3 + j)*3 + l]; mirrored: the input-gradient table (filter
// mirrored in all three axes).  One summation order for the per-layer and the batched pack: bit-identical tables.
__device__ __forceinline__ float wino3_u(const float *wp, int pz, int a, int b, bool mirrored) {
    const float G[4][3] = {{1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.f, 0.f, 1.f}};
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int l = 0; l < 3; l++) {
                const int t = mirrored ? ((2 - i) * 3 + (2 - j)) * 3 + (2 - l) : (i * 3 + j) * 3 + l;
                s += ((G[pz][i] * G[a][j]) * G[b][l]) * wp[t];
            }
    return s;
}

// one (pz, a, b, c, k) entry of uf (conv forward: reduce C, produce K) and ub (input gradient: reduce K, produce C)
__device__ __forceinline__ void pack_wino3_entry(const float *wp, float *__restrict__ uf, float *__restrict__ ub, int K,
                                                 int C, int k, int c, int pos) {
    const int b = pos & 3, a = (pos >> 2) & 3, pz = pos >> 4;
    if (uf) uf[u3idx(K, c >> 4, pz, a, b, (c >> 3) & 1, k, c & 7)] = wino3_u(wp, pz, a, b, false);
    if (ub) ub[u3idx(C, k >> 4, pz, a, b, (k >> 3) & 1, c, k & 7)] = wino3_u(wp, pz, a, b, true);
}

// batched pack (k_pack_batch, conv_wino.hip): tile = LDS [k 16][c 16][t 27] of one 16 x 16 block at (k0, c0)
__device__ __forceinline__ void pack_wino3_tile(const float *tile, float *__restrict__ uf, float *__restrict__ ub, int K, int C, int k0,
                                int c0, int tid) {
    const int q4 = tid >> 6, mid = (tid >> 2) & 15, l4 = tid & 3;
    // uf: c = c0 + q4 * 4 + l4, k = k0 + mid;  ub: k = k0 + q4 * 4 + l4, c = c0 + mid
    for (int pos = 0; pos < 64; pos++) {
        if (uf) {
            const int c = c0 + q4 * 4 + l4, k = k0 + mid;
            pack_wino3_entry(tile + mid * 432 + (q4 * 4 + l4) * 27, uf, nullptr, K, C, k, c, pos);
        }
        if (ub) {
            const int k = k0 + q4 * 4 + l4, c = c0 + mid;
            pack_wino3_entry(tile + (q4 * 4 + l4) * 432 + mid * 27, nullptr, ub, K, C, k, c, pos);
        }
    }
}

}  // namespace mvd
