// Layer normalization of a layer's input (include/currennt_hip.h, section Layer normalization; no counterpart in the reference):
// a marked layer's input products read a copy of the preceding layer's operand rows with zero mean and unit variance over the
// row's units, and the error the layer hands back passes the normalisation's Jacobian.  No gain, no bias: nothing is summed over
// frames, so there are no atomics and nothing order-dependent between workgroups.  gfx950 only.
//
//   layernorm_fwd_kernel   xn[N][Pp] (op) = (x[N][Pp] (op) - mean) * rstd on real frames, zeros elsewhere and in pad columns;
//                          rstd[N] (fp32) kept for the backward pass
//   layernorm_bwd_kernel   err[N][Pp] (fp32) = rstd * (g - mean(g) - xn * mean(g * xn)) in place on real frames, zeros elsewhere
// Both are row kernels bound by memory traffic: one 64-lane wave owns a row, a 256-thread workgroup four rows, a capped grid loops
// over rows.  A lane owns 16 bytes of every 64-lane trip across the row (G columns); the row is loaded once and held in
// registers across the statistics passes and the store (TRIPS = 1, 2, 4 or 8 trips, unrolled), and only a row wider than 2048
// columns is read again per pass (TRIPS = 0).  Per-lane partial sums are doubles, the wave sum is a __shfl_xor butterfly: every lane
// ends with the same bits.  The statistics run over the units of the reference layout (cn_unit_map.h), never over pad
// columns.  No LDS.
#include "cn_internal.h"

namespace cn {

__device__ __forceinline__ double ln_wave_sum(double s)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    return s;
}
// G consecutive elements of an operand row (F32: 4 floats, else 8 bf16: 16 bytes either way) from element offset `off`, widened
template <bool F32, int G>
__device__ __forceinline__ void ln_load_op(const void *p, long off, float (&v)[G])
{
    if constexpr (F32) {
        static_assert(G == 4, "16 bytes of fp32");
        const float4 q = *(const float4 *)((const float *)p + off);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if constexpr (G == 8) {
        const uint4 q = *(const uint4 *)((const unsigned short *)p + off);
        v[0] = bf16_lo(q.x); v[1] = bf16_hi(q.x); v[2] = bf16_lo(q.y); v[3] = bf16_hi(q.y);
        v[4] = bf16_lo(q.z); v[5] = bf16_hi(q.z); v[6] = bf16_lo(q.w); v[7] = bf16_hi(q.w);
    } else {
        static_assert(G == 4, "8 bytes of bf16 beside 16 bytes of fp32");
        const uint2 q = *(const uint2 *)((const unsigned short *)p + off);
        v[0] = bf16_lo(q.x); v[1] = bf16_hi(q.x); v[2] = bf16_lo(q.y); v[3] = bf16_hi(q.y);
    }
}
// ... and the 16-byte store of the forward kernel: one rounding to the operand type (none in fp32, to nearest even in bf16)
template <bool F32, int G>
__device__ __forceinline__ void ln_store_op(void *p, long off, const float (&v)[G])
{
    if constexpr (F32) *(float4 *)((float *)p + off) = make_float4(v[0], v[1], v[2], v[3]);
    else
        *(uint4 *)((unsigned short *)p + off) = make_uint4(bf16_bits(v[0]) | bf16_bits(v[1]) << 16, bf16_bits(v[2]) | bf16_bits(v[3]) << 16,
                                                           bf16_bits(v[4]) | bf16_bits(v[5]) << 16, bf16_bits(v[6]) | bf16_bits(v[7]) << 16);
}

// The column group of trip t for this lane: its first column c (clamped into the row, so that a lane past the row's end loads
// bytes that exist and counts none of them: no branch around a load) and the number of units among its G columns.
struct LnGroup { int c, cnt; bool inside; };
template <int G>
__device__ __forceinline__ LnGroup ln_group(const LnArgs &a, int t, int lane)
{
    const int c = (t * 64 + lane) * G;
    LnGroup g;
    g.inside = c < a.prev.Lp;
    g.c = g.inside ? c : a.prev.Lp - G;
    g.cnt = g.inside ? a.prev.units_in_group(c, G) : 0;
    return g;
}

template <bool F32, int TRIPS>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(LnArgs a, const char *__restrict__ pat, const void *__restrict__ x,
                                                            void *__restrict__ xn, float *__restrict__ rstd)
{
    constexpr int G = F32 ? 4 : 8;
    constexpr bool HELD = TRIPS > 0;
    constexpr int NT = HELD ? TRIPS : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt = HELD ? TRIPS : (a.prev.Lp + 64 * G - 1) / (64 * G);
    const double inv_p = 1.0 / (double)a.prev.L;
    LnGroup grp[NT];                                      // (HELD: the same for every row)
    if constexpr (HELD) {
#pragma unroll
        for (int t = 0; t < NT; ++t) grp[t] = ln_group<G>(a, t, lane);
    }
    auto group = [&](int t) { if constexpr (HELD) return grp[t]; else return ln_group<G>(a, t, lane); };
    for (long row = (long)blockIdx.x * 4 + wave; row < a.N; row += (long)gridDim.x * 4) {
        const long base = row * a.prev.Lp;
        if (pat[row] == 0) {                              // dummy frame or pad slot (the wave's rows are its own: a uniform branch)
            const float z[G] = {};
#pragma unroll NT
            for (int t = 0; t < (HELD ? NT : nt); ++t) {
                const LnGroup g = group(t);
                if (g.inside) ln_store_op<F32, G>(xn, base + g.c, z);
            }
            if (lane == 0) rstd[row] = 0.f;
            continue;
        }
        float v[NT][G];
        // pass 1: the mean
        double s = 0.0;
#pragma unroll NT
        for (int t = 0; t < (HELD ? NT : nt); ++t) {
            const LnGroup g = group(t);
            float (&w)[G] = v[HELD ? t : 0];
            ln_load_op<F32, G>(x, base + g.c, w);
#pragma unroll
            for (int k = 0; k < G; ++k) s += k < g.cnt ? (double)w[k] : 0.0;
        }
        const double mean = ln_wave_sum(s) * inv_p;
        // pass 2: the variance about that mean
        double q = 0.0;
#pragma unroll NT
        for (int t = 0; t < (HELD ? NT : nt); ++t) {
            const LnGroup g = group(t);
            float (&w)[G] = v[HELD ? t : 0];
            if constexpr (!HELD) ln_load_op<F32, G>(x, base + g.c, w);
#pragma unroll
            for (int k = 0; k < G; ++k) { const double d = (double)w[k] - mean; q += k < g.cnt ? d * d : 0.0; }
        }
        const double var = ln_wave_sum(q) * inv_p;
        const float mean_f = (float)mean, rstd_f = (float)(1.0 / sqrt(var + (double)a.eps));
        // the normalised copy: two fp32 operations, each rounded to nearest, then the rounding to the operand type
#pragma unroll NT
        for (int t = 0; t < (HELD ? NT : nt); ++t) {
            const LnGroup g = group(t);
            float (&w)[G] = v[HELD ? t : 0];
            if constexpr (!HELD) ln_load_op<F32, G>(x, base + g.c, w);
            float o[G];
#pragma unroll
            for (int k = 0; k < G; ++k) o[k] = k < g.cnt ? __fmul_rn(__fsub_rn(w[k], mean_f), rstd_f) : 0.f;
            if (g.inside) ln_store_op<F32, G>(xn, base + g.c, o);
        }
        if (lane == 0) rstd[row] = rstd_f;
    }
}

// err: dL/d xn as the layer's K8 (and its dropout mask) left it, fp32 [N][Pp]; rewritten in place as dL/dx.  Four columns per lane
// and trip: 16 bytes of err, 16 (F32) or 8 bytes of xn.
template <bool F32, int TRIPS>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(LnArgs a, const char *__restrict__ pat, const void *__restrict__ xn,
                                                            const float *__restrict__ rstd, float *__restrict__ err)
{
    constexpr int G = 4;
    constexpr bool HELD = TRIPS > 0;
    constexpr int NT = HELD ? TRIPS : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt = HELD ? TRIPS : (a.prev.Lp + 64 * G - 1) / (64 * G);
    const double inv_p = 1.0 / (double)a.prev.L;
    LnGroup grp[NT];
    if constexpr (HELD) {
#pragma unroll
        for (int t = 0; t < NT; ++t) grp[t] = ln_group<G>(a, t, lane);
    }
    auto group = [&](int t) { if constexpr (HELD) return grp[t]; else return ln_group<G>(a, t, lane); };
    for (long row = (long)blockIdx.x * 4 + wave; row < a.N; row += (long)gridDim.x * 4) {
        const long base = row * a.prev.Lp;
        if (pat[row] == 0) {
#pragma unroll NT
            for (int t = 0; t < (HELD ? NT : nt); ++t) {
                const LnGroup g = group(t);
                if (g.inside) *(float4 *)(err + base + g.c) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            continue;
        }
        float e[NT][G], h[NT][G];
        double s1 = 0.0, s2 = 0.0;                         // sum of g and of g * xn over the row's units
#pragma unroll NT
        for (int t = 0; t < (HELD ? NT : nt); ++t) {
            const LnGroup g = group(t);
            float (&we)[G] = e[HELD ? t : 0];
            float (&wh)[G] = h[HELD ? t : 0];
            ln_load_op<true, G>(err, base + g.c, we);
            ln_load_op<F32, G>(xn, base + g.c, wh);
#pragma unroll
            for (int k = 0; k < G; ++k) {
                s1 += k < g.cnt ? (double)we[k] : 0.0;
                s2 += k < g.cnt ? (double)we[k] * (double)wh[k] : 0.0;
            }
        }
        const float m1 = (float)(ln_wave_sum(s1) * inv_p), m2 = (float)(ln_wave_sum(s2) * inv_p), r = rstd[row];
#pragma unroll NT
        for (int t = 0; t < (HELD ? NT : nt); ++t) {
            const LnGroup g = group(t);
            float (&we)[G] = e[HELD ? t : 0];
            float (&wh)[G] = h[HELD ? t : 0];
            if constexpr (!HELD) { ln_load_op<true, G>(err, base + g.c, we); ln_load_op<F32, G>(xn, base + g.c, wh); }
            float o[G];
#pragma unroll
            for (int k = 0; k < G; ++k) o[k] = k < g.cnt ? __fmul_rn(r, __fsub_rn(__fsub_rn(we[k], m1), __fmul_rn(wh[k], m2))) : 0.f;
            if (g.inside) *(float4 *)(err + base + g.c) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// trips of 64 lanes x G columns across a row of Pp columns, rounded up to a count the kernels are unrolled for; 0: a row wider
// than LN_HELD_COLUMNS, which is not held in registers (32 floats per lane and array at the most)
#define LN_HELD_COLUMNS 2048
static int ln_trips(int Pp, int G)
{
    for (int t = 1; t * 64 * G <= LN_HELD_COLUMNS; t *= 2) if (Pp <= t * 64 * G) return t;
    return 0;
}
static int ln_blocks(int N) { const int b = (N + 3) / 4; return b > 2048 ? 2048 : b; }

#define LN_LAUNCH(kernel, F32, ...)                                                                                                  \
    switch (trips) {                                                                                                                 \
    case 1: hipLaunchKernelGGL((kernel<F32, 1>), dim3(blocks), dim3(256), 0, s, __VA_ARGS__); break;                                   \
    case 2: hipLaunchKernelGGL((kernel<F32, 2>), dim3(blocks), dim3(256), 0, s, __VA_ARGS__); break;                                   \
    case 4: hipLaunchKernelGGL((kernel<F32, 4>), dim3(blocks), dim3(256), 0, s, __VA_ARGS__); break;                                   \
    case 8: hipLaunchKernelGGL((kernel<F32, 8>), dim3(blocks), dim3(256), 0, s, __VA_ARGS__); break;                                   \
    default: hipLaunchKernelGGL((kernel<F32, 0>), dim3(blocks), dim3(256), 0, s, __VA_ARGS__); break;                                  \
    }

void launch_layernorm_fwd(hipStream_t s, bool f32, const LnArgs &a, const char *pat, const void *x, void *xn, float *rstd)
{
    if (a.N <= 0) return;
    const int blocks = ln_blocks(a.N), trips = ln_trips(a.prev.Lp, f32 ? 4 : 8);
    if (f32) { LN_LAUNCH(layernorm_fwd_kernel, true, a, pat, x, xn, rstd) }
    else     { LN_LAUNCH(layernorm_fwd_kernel, false, a, pat, x, xn, rstd) }
}
void launch_layernorm_bwd(hipStream_t s, bool f32, const LnArgs &a, const char *pat, const void *xn, const float *rstd, float *err)
{
    if (a.N <= 0) return;
    const int blocks = ln_blocks(a.N), trips = ln_trips(a.prev.Lp, 4);
    if (f32) { LN_LAUNCH(layernorm_bwd_kernel, true, a, pat, xn, rstd, err) }
    else     { LN_LAUNCH(layernorm_bwd_kernel, false, a, pat, xn, rstd, err) }
}
#undef LN_LAUNCH

}  // namespace cn
