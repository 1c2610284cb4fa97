// Strided context layers: a context layer that keeps every S-th frame and so starts a new, shorter time axis (include/
// currennt_hip.h, section Strided context layers).  Kernels of their own beside cn_context.hip's, whose stride-1 code objects keep
// their code.  gfx950 only.
//
//   stride_axis_kernel     the layer's own axis from the parent's slot lengths len_s: n_s = ceil(len_s / S), the derived pattern
//                          types (FIRST for j = 0, LAST for j = n_s - 1 > 0, NORMAL between, NONE for j >= n_s and in pad slots)
//                          and the classes of parent row S * j (-1 elsewhere); every row of T' * PSp written
//   stride_targets_kernel  the target rows of base row rate * j for j < n_s, zero rows elsewhere
//   stride_fwd_kernel      out[j][s][b * P + u] (op) = x[clamp(S * j + (b - L) * D, 0, len_s - 1)][s][u] (op), bits copied; zeros
//                          on the rows j >= n_s and in pad columns
//   stride_bwd_kernel      dx[ts][s][u] (fp32) = the sum of e[j][s][b * P + u] over the (b, j) that read parent frame ts, b
//                          ascending, then j ascending, single fp32 additions from +0.0f; +0.0 for a frame nobody reads; zeros
//                          on every other row of the parent's fraction and in pad columns
// Streaming kernels with cn_context.hip's thread map: a thread owns one 16-byte piece of one row (RUN: loaded as one piece where
// blocks and directions are whole pieces; otherwise put together from element loads), grid-stride loops, no LDS, no atomics.
#include <type_traits>

#include "cn_internal.h"

namespace cn {

enum { STR_NONE = 0, STR_FIRST = 1, STR_NORMAL = 2, STR_LAST = 3 };       // (Types.hpp:30-33)

__global__ __launch_bounds__(256) void stride_axis_kernel(int S, int Tout, int PSp, const int *__restrict__ len, const int *__restrict__ tcls,
                                                          int *__restrict__ nlen, char *__restrict__ npat, int *__restrict__ ntcls)
{
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    const long total = (long)Tout * PSp;
    for (long idx = tid; idx < total; idx += nth) {
        const int j = (int)(idx / PSp), s = (int)(idx % PSp);
        const int n = (len[s] + S - 1) / S;
        if (j == 0) nlen[s] = n;
        npat[idx] = (char)(j >= n ? STR_NONE : j == 0 ? STR_FIRST : j == n - 1 ? STR_LAST : STR_NORMAL);
        ntcls[idx] = j < n ? tcls[(long)S * j * PSp + s] : -1;
    }
}

__global__ __launch_bounds__(256) void stride_targets_kernel(int rate, int Tout, int PSp, int W, const int *__restrict__ nlen,
                                                             const float *__restrict__ src, float *__restrict__ tgt)
{
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    const long total = (long)Tout * PSp * W;
    for (long idx = tid; idx < total; idx += nth) {
        const long r = idx / W; const int w = (int)(idx % W);
        const int j = (int)(r / PSp), s = (int)(r % PSp);
        tgt[idx] = j < nlen[s] ? src[((long)rate * j * PSp + s) * W + w] : 0.f;
    }
}

// the parent frame of slot s that block b of frame j reads; len >= 1
__device__ __forceinline__ int stride_src(const StrideArgs &a, int j, int b, int len) { return max(0, min(a.S * j + (b - a.left) * a.dil, len - 1)); }

template <bool F32, int VEC, bool RUN>
__global__ __launch_bounds__(256) void stride_fwd_kernel(StrideArgs a, const int *__restrict__ len, const void *__restrict__ x, void *__restrict__ out)
{
    typedef typename std::conditional<F32, unsigned, unsigned short>::type op_t;      // (the bits of an operand: nothing is rounded)
    static_assert(VEC * sizeof(op_t) == 16, "a piece is 16 bytes");
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    const int pieces = a.Lp / VEC, width = a.B * a.prev.L;
    const long total = (long)a.Tout * a.PSp * pieces;
    for (long idx = tid; idx < total; idx += nth) {
        const long n = idx / pieces; const int c0 = (int)(idx % pieces) * VEC;
        const int j = (int)(n / a.PSp), s = (int)(n % a.PSp);
        const int ln = len[s];
        const bool live = (long)a.S * j < ln && c0 < width;      // (j < n_s = ceil(len_s / S))
        int b = 0, u = 0;                                  // block and unit of the piece's first column
        if (live) { b = c0 / a.prev.L; u = c0 - b * a.prev.L; }
        if constexpr (RUN) {
            uint4 o = make_uint4(0u, 0u, 0u, 0u);
            if (live) o = *(const uint4 *)((const op_t *)x + ((long)stride_src(a, j, b, ln) * a.PSp + s) * a.prev.Lp + a.prev.col(u));
            *(uint4 *)((op_t *)out + n * a.Lp + c0) = o;
        } else {
            union { op_t e[VEC]; uint4 q; } v;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                op_t w = 0;
                if (live && c0 + i < width) {
                    w = ((const op_t *)x)[((long)stride_src(a, j, b, ln) * a.PSp + s) * a.prev.Lp + a.prev.col(u)];
                    if (++u == a.prev.L) { u = 0; ++b; }
                }
                v.e[i] = w;
            }
            *(uint4 *)((op_t *)out + n * a.Lp + c0) = v.q;
        }
    }
}

template <bool RUN>
__global__ __launch_bounds__(256) void stride_bwd_kernel(StrideArgs a, const int *__restrict__ len, const float *__restrict__ e, float *__restrict__ dx)
{
    constexpr int VEC = 4;                                  // a piece is four fp32
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    const int pieces = a.prev.Lp / VEC;
    const long total = (long)a.Tin * a.PSp * pieces;
    for (long idx = tid; idx < total; idx += nth) {
        const long n = idx / pieces; const int c0 = (int)(idx % pieces) * VEC;
        const int t = (int)(n / a.PSp), s = (int)(n % a.PSp);
        const int ln = len[s];
        const int nj = (ln + a.S - 1) / a.S;                // n_s
        const int u0 = a.prev.unit(c0);
        const int cnt = a.prev.units_in_group(c0, VEC);
        float acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
        if (t < ln && cnt > 0) {
            for (int b = 0; b < a.B; ++b) {
                // the frames j < n_s with clamp(S * j + o, 0, len - 1) == t: inside the sequence the one j with S * j == t - o,
                // if S divides it; the runs that the clamp folds onto the first and the last frame
                const int o = (b - a.left) * a.dil, d = t - o;
                const int jlo = (t == 0 || d <= 0) ? 0 : (d + a.S - 1) / a.S;
                const int jhi = t == ln - 1 ? nj - 1 : (d < 0 ? -1 : min(d / a.S, nj - 1));
                for (int j = jlo; j <= jhi; ++j) {
                    const float *p = e + ((long)j * a.PSp + s) * a.Lp + b * a.prev.L + u0;
                    if constexpr (RUN) {
                        const float4 v = *(const float4 *)p;
                        acc[0] = __fadd_rn(acc[0], v.x); acc[1] = __fadd_rn(acc[1], v.y); acc[2] = __fadd_rn(acc[2], v.z); acc[3] = __fadd_rn(acc[3], v.w);
                    } else {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) if (i < cnt) acc[i] = __fadd_rn(acc[i], p[i]);
                    }
                }
            }
        }
        *(float4 *)(dx + n * a.prev.Lp + c0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}

static int stride_blocks(long work) { long b = (work + 255) / 256; return (int)(b > 2048 ? 2048 : b < 1 ? 1 : b); }
static bool stride_runs(const StrideArgs &a, int vec) { return a.prev.L % vec == 0 && a.prev.H % vec == 0; }

void launch_stride_axis(hipStream_t s, int S, int Tout, int PSp, const int *len, const int *tcls, int *nlen, char *npat, int *ntcls)
{
    if ((long)Tout * PSp <= 0) return;
    hipLaunchKernelGGL(stride_axis_kernel, dim3(stride_blocks((long)Tout * PSp)), dim3(256), 0, s, S, Tout, PSp, len, tcls, nlen, npat, ntcls);
}

void launch_stride_targets(hipStream_t s, int rate, int Tout, int PSp, int W, const int *nlen, const float *src, float *tgt)
{
    const long total = (long)Tout * PSp * W; if (total <= 0) return;
    hipLaunchKernelGGL(stride_targets_kernel, dim3(stride_blocks(total)), dim3(256), 0, s, rate, Tout, PSp, W, nlen, src, tgt);
}

void launch_stride_fwd(hipStream_t s, bool f32, const StrideArgs &a, const int *len, const void *x, void *out)
{
    const long rows = (long)a.Tout * a.PSp; if (rows <= 0) return;
    const int vec = f32 ? 4 : 8;
    const bool runs = stride_runs(a, vec) && ((size_t)x & 15) == 0;
    const int blocks = stride_blocks(rows * (a.Lp / vec));
#define CN_STRIDE_FWD(F32, VEC, RUN) hipLaunchKernelGGL((stride_fwd_kernel<F32, VEC, RUN>), dim3(blocks), dim3(256), 0, s, a, len, x, out)
    if (f32) { if (runs) CN_STRIDE_FWD(true, 4, true); else CN_STRIDE_FWD(true, 4, false); }
    else     { if (runs) CN_STRIDE_FWD(false, 8, true); else CN_STRIDE_FWD(false, 8, false); }
#undef CN_STRIDE_FWD
}

void launch_stride_bwd(hipStream_t s, const StrideArgs &a, const int *len, const float *e, float *dx)
{
    const long rows = (long)a.Tin * a.PSp; if (rows <= 0) return;
    const bool runs = stride_runs(a, 4) && ((size_t)e & 15) == 0;
    const int blocks = stride_blocks(rows * (a.prev.Lp / 4));
    if (runs) hipLaunchKernelGGL(stride_bwd_kernel<true>, dim3(blocks), dim3(256), 0, s, a, len, e, dx);
    else      hipLaunchKernelGGL(stride_bwd_kernel<false>, dim3(blocks), dim3(256), 0, s, a, len, e, dx);
}

}  // namespace cn
