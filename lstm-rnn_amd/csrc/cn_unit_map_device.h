// Device functions that map a unit of the reference layout to its column in a layer's padded rows and back.  Dense layers, the
// input layer and a one-directional lstm keep unit u at column u (H = 0 says "dense"); a blstm puts direction d's unit j at
// d * Hp + j.  Included by cn_residual.hip (the sum matches the units of two layers) and cn_layernorm.hip (a row's statistics are
// taken over its units, never over pad columns).
#pragma once

#include <hip/hip_runtime.h>

namespace cn {

// column of unit u in a layer's padded rows (H = 0: dense)
__device__ __forceinline__ int res_col(int u, int H, int Hp) { return H == 0 ? u : (u / H) * Hp + u % H; }
// unit of padded column c, or -1 for a pad column
__device__ __forceinline__ int res_unit(int c, int L, int H, int Hp, int dirs)
{
    if (H == 0) return c < L ? c : -1;
    const int d = c / Hp, j = c % Hp;
    return (d < dirs && j < H) ? d * H + j : -1;
}
// units among the G columns that start at c (a multiple of G; Hp and every row width are multiples of 32, so the G columns lie in
// one direction and the units among them come first)
__device__ __forceinline__ int res_units_in_group(int c, int G, int L, int H, int Hp, int dirs)
{
    int cnt;
    if (H == 0) cnt = L - c;
    else { const int d = c / Hp, j = c % Hp; cnt = d < dirs ? H - j : 0; }
    return max(0, min(cnt, G));
}
// a bf16 pair in one 32-bit word, widened; and one float rounded to bf16 bits (to nearest even)
__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xFFFF0000u); }
__device__ __forceinline__ unsigned bf16_bits(float v) { return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)v); }

}  // namespace cn
