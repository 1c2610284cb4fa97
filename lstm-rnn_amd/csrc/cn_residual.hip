// Residual connections between layers (include/currennt_hip.h, section Residual connections; no counterpart in the reference):
// what a marked layer's followers read is the layer's own output, its "branch", plus the preceding layer's output.  gfx950 only.
//
//   residual_fwd_kernel   sum[N][Lp] (op)  = branch[N][Lp] (op) + x[N][xLp] (op) on real frames, the branch elsewhere; pad columns 0
//   residual_bwd_kernel   prev_err[N][xLp] (fp32) += e[N][Lp] (fp32) on real frames
// Both are streaming kernels: grid-stride loops, no LDS.  Units are matched in the reference layout (unit u of both layers); the
// padded column of a unit depends on the layer's kind (cn_unit_map.h).  Where the two column maps coincide (ResArgs::same_map) a thread
// owns 16 bytes of one row (VEC); otherwise one element, whose partner it looks up (the mapped path).
#include "cn_internal.h"

namespace cn {

// one 32-bit word of two bf16: element k0 (low half) and k0 + 1 of a group with cnt units; real: add x, else keep the branch
__device__ __forceinline__ unsigned res_word(unsigned b, unsigned x, int k0, int cnt, bool real)
{
    float lo = bf16_lo(b), hi = bf16_hi(b);
    if (real) { lo = __fadd_rn(lo, bf16_lo(x)); hi = __fadd_rn(hi, bf16_hi(x)); }
    return (k0 < cnt ? bf16_bits(lo) : 0u) | (k0 + 1 < cnt ? bf16_bits(hi) << 16 : 0u);
}

template <bool F32, bool VEC>
__global__ __launch_bounds__(256) void residual_fwd_kernel(ResArgs a, const char *__restrict__ pat, const void *__restrict__ branch,
                                                           const void *__restrict__ x, void *__restrict__ sum)
{
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    if constexpr (VEC) {
        constexpr int G = F32 ? 4 : 8;                    // elements in 16 bytes
        const int q = a.own.Lp / G;
        for (long idx = tid; idx < (long)a.N * q; idx += nth) {
            const long row = idx / q; const int c = (int)(idx % q) * G;
            const int cnt = a.own.units_in_group(c, G);
            const bool real = pat[row] != 0;
            uint4 o = make_uint4(0u, 0u, 0u, 0u);
            if (cnt > 0) {
                if constexpr (F32) {
                    float4 b = *(const float4 *)((const float *)branch + row * a.own.Lp + c);
                    if (real) {
                        const float4 v = *(const float4 *)((const float *)x + row * a.prev.Lp + c);
                        b.x = __fadd_rn(b.x, v.x); b.y = __fadd_rn(b.y, v.y); b.z = __fadd_rn(b.z, v.z); b.w = __fadd_rn(b.w, v.w);
                    }
                    o.x = __float_as_uint(b.x);
                    o.y = cnt > 1 ? __float_as_uint(b.y) : 0u; o.z = cnt > 2 ? __float_as_uint(b.z) : 0u; o.w = cnt > 3 ? __float_as_uint(b.w) : 0u;
                } else {
                    const uint4 b = *(const uint4 *)((const unsigned short *)branch + row * a.own.Lp + c);
                    uint4 v = make_uint4(0u, 0u, 0u, 0u);
                    if (real) v = *(const uint4 *)((const unsigned short *)x + row * a.prev.Lp + c);
                    o.x = res_word(b.x, v.x, 0, cnt, real); o.y = res_word(b.y, v.y, 2, cnt, real);
                    o.z = res_word(b.z, v.z, 4, cnt, real); o.w = res_word(b.w, v.w, 6, cnt, real);
                }
            }
            if constexpr (F32) *(uint4 *)((float *)sum + row * a.own.Lp + c) = o;
            else               *(uint4 *)((unsigned short *)sum + row * a.own.Lp + c) = o;
        }
    } else {
        for (long idx = tid; idx < (long)a.N * a.own.Lp; idx += nth) {
            const long row = idx / a.own.Lp; const int c = (int)(idx % a.own.Lp);
            const int u = a.own.unit(c);
            float v = 0.f;
            if (u >= 0) {
                const long xi = row * a.prev.Lp + a.prev.col(u);
                if constexpr (F32) {
                    v = ((const float *)branch)[idx];
                    if (pat[row] != 0) v = __fadd_rn(v, ((const float *)x)[xi]);
                } else {
                    v = bf16_lo(((const unsigned short *)branch)[idx]);
                    if (pat[row] != 0) v = __fadd_rn(v, bf16_lo(((const unsigned short *)x)[xi]));
                }
            }
            if constexpr (F32) ((float *)sum)[idx] = v; else ((unsigned short *)sum)[idx] = (unsigned short)bf16_bits(v);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void residual_bwd_kernel(ResArgs a, const char *__restrict__ pat, const float *__restrict__ e,
                                                           float *__restrict__ prev_err)
{
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    if constexpr (VEC) {
        const int q = a.own.Lp / 4;
        for (long idx = tid; idx < (long)a.N * q; idx += nth) {
            const long row = idx / q; const int c = (int)(idx % q) * 4;
            const int cnt = a.own.units_in_group(c, 4);
            if (cnt <= 0 || pat[row] == 0) continue;
            const float4 v = *(const float4 *)(e + row * a.own.Lp + c);
            float4 *p = (float4 *)(prev_err + row * a.prev.Lp + c);
            float4 s = *p;
            s.x = __fadd_rn(s.x, v.x);
            if (cnt > 1) s.y = __fadd_rn(s.y, v.y);
            if (cnt > 2) s.z = __fadd_rn(s.z, v.z);
            if (cnt > 3) s.w = __fadd_rn(s.w, v.w);
            *p = s;
        }
    } else {
        for (long idx = tid; idx < (long)a.N * a.own.Lp; idx += nth) {
            const long row = idx / a.own.Lp; const int c = (int)(idx % a.own.Lp);
            const int u = a.own.unit(c);
            if (u < 0 || pat[row] == 0) continue;
            float *p = prev_err + row * a.prev.Lp + a.prev.col(u);
            *p = __fadd_rn(*p, e[idx]);
        }
    }
}

static int residual_blocks(long work) { long b = (work + 255) / 256; return (int)(b > 2048 ? 2048 : b); }

void launch_residual_fwd(hipStream_t s, bool f32, const ResArgs &a, const char *pat, const void *branch, const void *x, void *sum)
{
    if (a.N <= 0) return;
    if (a.same_map) {
        const int blocks = residual_blocks((long)a.N * (a.own.Lp / (f32 ? 4 : 8)));
        if (f32) hipLaunchKernelGGL((residual_fwd_kernel<true, true>), dim3(blocks), dim3(256), 0, s, a, pat, branch, x, sum);
        else     hipLaunchKernelGGL((residual_fwd_kernel<false, true>), dim3(blocks), dim3(256), 0, s, a, pat, branch, x, sum);
    } else {
        const int blocks = residual_blocks((long)a.N * a.own.Lp);
        if (f32) hipLaunchKernelGGL((residual_fwd_kernel<true, false>), dim3(blocks), dim3(256), 0, s, a, pat, branch, x, sum);
        else     hipLaunchKernelGGL((residual_fwd_kernel<false, false>), dim3(blocks), dim3(256), 0, s, a, pat, branch, x, sum);
    }
}
void launch_residual_bwd(hipStream_t s, const ResArgs &a, const char *pat, const float *e, float *prev_err)
{
    if (a.N <= 0) return;
    if (a.same_map) hipLaunchKernelGGL(residual_bwd_kernel<true>, dim3(residual_blocks((long)a.N * (a.own.Lp / 4))), dim3(256), 0, s, a, pat, e, prev_err);
    else            hipLaunchKernelGGL(residual_bwd_kernel<false>, dim3(residual_blocks((long)a.N * a.own.Lp)), dim3(256), 0, s, a, pat, e, prev_err);
}

}  // namespace cn
