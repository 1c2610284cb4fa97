// Device helpers shared by the GEMM kernels (cn_gemm.hip, cn_gemm_big.hip, cn_gemm_nt_mid.hip, cn_gemm_nt_panel.hip,
// cn_gemm_tn_big.hip): the reference's output activation, one K-group of a 32x32 MFMA tile product, the tile order, the C/D
// register map of the 32x32 MFMA, the store of one result row and the buffer resource of an operand.  What differs from kernel
// to kernel for a reason -- the k-tile bodies, the fill addresses, the counted waits -- stays in the kernels.
#pragma once

#include "cn_internal.h"
#include "cn_lstm_device.h"      // vector types, split_bf16

namespace cn {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

__device__ __forceinline__ float act_apply(int act, float x)
{
    // activation_functions/Logistic.cuh:33-44, Tanh.cuh:33-36 (tanh(x) = 2*logistic(2x) - 1)
    if (act == ACT_IDENTITY) return x;
    float z = (act == ACT_TANH) ? 2.0f * x : x;
    float s;
    if (z < 88.722839f) s = (z > -88.722839f) ? 1.0f / (1.0f + __expf(-z)) : 0.0f;
    else s = 1.0f;
    return (act == ACT_TANH) ? 2.0f * s - 1.0f : s;
}

// one K-group (32 bytes of K per row: 16 bf16 or 8 fp32) of a 32x32 tile product
template <bool F32>
__device__ __forceinline__ void mma32(f32x16 &acc, const u32x4 &a, const u32x4 &b)
{
    if constexpr (F32) {
        // K order inside the group is permuted identically for A and B (lane half h holds
        // k = 4h..4h+3), which leaves the dot product unchanged.
        // (bit_cast the whole vector: a bit_cast of a single ext_vector element picks element 0)
        const f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[i], acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                      __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
}

// split-bf16 product of one 16-element K-group of a 32x32 tile (P_X3): three bf16 MFMAs, small terms first
__device__ __forceinline__ void mma32_x3(f32x16 &acc, const u32x4 &ah, const u32x4 &al, const u32x4 &bh, const u32x4 &bl)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al), __builtin_bit_cast(bf16x8, bh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bl), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bh), acc, 0, 0, 0);
}
// four fp32 -> 4 bf16 hi and 4 bf16 lo (8 bytes each)
__device__ __forceinline__ void split4(const u32x4 &x, u32x2 &hi, u32x2 &lo)
{
    const f32x4 f = __builtin_bit_cast(f32x4, x);
    bf16x4 h, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) { __bf16 a, b; split_bf16(f[i], a, b); h[i] = a; l[i] = b; }
    hi = __builtin_bit_cast(u32x2, h); lo = __builtin_bit_cast(u32x2, l);
}

// ---- tile order ---------------------------------------------------------------------------------------------------
// XCD-aware tile order: blocks b and b+8 share an XCD (and its L2); give each XCD a contiguous
// run of tiles so the N-tiles of one A panel hit the same L2 (bijective remap).
__device__ __forceinline__ int xcd_tile_order(int bid, int nwg)
{
    const int q = nwg / 8, r = nwg % 8, x = bid % 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bid / 8;
}

// the same order seen from XCD x (gemm_nt_big8_kernel walks its XCD's run itself): tile start + i is what block x + 8 i gets above.
// (A second statement of the arithmetic, kept beside the first: built on one another, either form changed the code of every kernel.)
__device__ __forceinline__ void xcd_run(int x, int nwg, int &start, int &len)
{
    const int q = nwg / 8, r = nwg % 8;
    len = q + (x < r ? 1 : 0);
    start = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
}

// ... and inside an XCD's run, tiles in groups of GROUP_M tile rows walked column by column: the workgroups an XCD runs at a
// time then share GROUP_M A panels and a few B panels in its L2 instead of one A panel and every B panel (B is the whole weight
// matrix and does not fit the 4 MB L2: with row-major order every tile row streamed it from the Infinity Cache again)
template <int GROUP_M, int BM, int BN>
__device__ __forceinline__ void grouped_tile(int bid, int tiles_m, int tiles_n, int &m0, int &n0)
{
    const int per_group = GROUP_M * tiles_n, grp = bid / per_group, first_m = grp * GROUP_M;
    const int gm = min(GROUP_M, tiles_m - first_m), in_grp = bid - grp * per_group;
    m0 = (first_m + in_grp % gm) * BM; n0 = (in_grp / gm) * BN;
}

// ---- results ------------------------------------------------------------------------------------------------------
// C/D map of the 32x32 MFMA: accumulator register r of lane (fr = lane & 31, fh = lane >> 5) is row mfma32_row(r, fh),
// column fr of the block (row0: the block's first row, added in front so that the sum keeps the order the kernels had)
__host__ __device__ constexpr int mfma32_row(int r, int fh, int row0 = 0) { return row0 + (r & 3) + 8 * (r >> 2) + 4 * fh; }

// four columns of one result row: bias and activation, then the fp32 result and / or its operand-type copy (F32COPY: fp32)
template <bool F32COPY>
__device__ __forceinline__ void store_out4(const GemmNT &p, long m, int n, f32x4 v, const f32x4 &bias4)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = act_apply(p.act, v[e] + bias4[e]);
    if (p.C) *(f32x4 *)(p.C + m * p.ldc + n) = v;
    if (p.C2) {
        if constexpr (F32COPY) *(f32x4 *)((float *)p.C2 + m * p.ldc2 + n) = v;
        else {
            const bf16x4 hh = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
            *(bf16x4 *)((__bf16 *)p.C2 + m * p.ldc2 + n) = hh;
        }
    }
}

// ---- operands -----------------------------------------------------------------------------------------------------
// raw buffer resource over [base, base + bytes): loads past the end return zeros, stores past it are dropped
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_resource(const void *base, long bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, (int)(unsigned)bytes, 0x00020000);
}

// the fragment registers of the one-statement k-tile bodies (gemm_nt_mid_kernel, gemm_tn_big_kernel), as a clobber list
#define CN_FRAG_V200_247                                                                                                        \
    "v200", "v201", "v202", "v203", "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", \
    "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223", "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", \
    "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247"

// ---- split-K groups -----------------------------------------------------------------------------------------------
// which product of a grouped launch block `bid` belongs to (first_block: GROUP + 1 entries, unused products start at INT_MAX)
template <int N>
__device__ __forceinline__ int tn_group_member(const int (&first_block)[N], int bid)
{
    int gi = 0;
#pragma unroll
    for (int i = 1; i < N - 1; ++i) if (bid >= first_block[i]) gi = i;
    return gi;
}

}  // namespace cn
