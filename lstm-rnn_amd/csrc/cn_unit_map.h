// Where the units of a layer lie in its padded rows: the one statement of that map, read by host and device code alike (hipcc
// compiles the functions for both; a plain C++ compiler, as tests/unit_map_main.cpp and tests/noise_unpack_main.cpp use, for
// the host).
//
// A row is Lp columns wide and holds the layer's L units of the reference layout; every other column is pad and holds zeros.
//   H = 0   unit u at column u: a dense layer, the input layer, a context layer.  (A one-directional lstm says H = L, Hp = Lp,
//           dirs = 1, which is the same map.)
//   H > 0   dirs directions of H units each, Hp columns apart: direction d's unit j, unit d * H + j, at column d * Hp + j (a blstm)
// Lp and Hp are multiples of 32 (cn_layer_create*), so G <= 32 columns that start at a multiple of G -- one thread's 16 bytes --
// lie in one direction, and the units among them are the group's first columns: consecutive units, the pad behind them.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define CN_UNIT_MAP_FN __host__ __device__ __forceinline__
#else
#define CN_UNIT_MAP_FN inline
#endif

namespace cn {

struct UnitMap {
    int L, Lp, H, Hp, dirs;
    // column of unit u
    CN_UNIT_MAP_FN int col(int u) const { return H == 0 ? u : (u / H) * Hp + u % H; }
    // unit of column c, or -1 for a pad column
    CN_UNIT_MAP_FN int unit(int c) const
    {
        if (H == 0) return c < L ? c : -1;
        const int d = c / Hp, j = c % Hp;
        return (d < dirs && j < H) ? d * H + j : -1;
    }
    // units among the G columns that start at c (a multiple of G): they are the columns c .. c + count - 1
    CN_UNIT_MAP_FN int units_in_group(int c, int G) const
    {
        int cnt;
        if (H == 0) cnt = L - c;
        else { const int d = c / Hp, j = c % Hp; cnt = d < dirs ? H - j : 0; }
        if (cnt > G) cnt = G;
        return cnt < 0 ? 0 : cnt;
    }
};

#ifdef __HIPCC__
// a bf16 pair in one 32-bit word, widened; and one float rounded to bf16 bits (to nearest even)
__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xFFFF0000u); }
__device__ __forceinline__ unsigned bf16_bits(float v) { return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)v); }
#endif

}  // namespace cn
