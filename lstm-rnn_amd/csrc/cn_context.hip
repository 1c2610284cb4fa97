// Context layers: a hidden layer that splices its predecessor's neighbouring frames and, with a stride S > 1, keeps every S-th
// frame and so starts a new, shorter time axis (include/currennt_hip.h, sections Context layers and Strided context layers; no
// counterpart in the reference, which splices the input patterns only).  S = 1 is the plain layer: it lies in its predecessor's
// axis, n_s = len_s and Tout = Tin.  gfx950 only.
//
//   context_len_kernel     len[s] = frames of slot s whose pattern type is not NONE, for every slot of a time step (pad slots: 0)
//   stride_axis_kernel     (S > 1 only) the layer's own axis from the parent's slot lengths len_s: n_s = ceil(len_s / S), the
//                          derived pattern types (FIRST for j = 0, LAST for j = n_s - 1 > 0, NORMAL between, NONE for j >= n_s and
//                          in pad slots) and the classes of parent row S * j (-1 elsewhere); every row of T' * PSp written
//   stride_targets_kernel  (S > 1 only) the target rows of base row rate * j for j < n_s, zero rows elsewhere
//   context_fwd_kernel     out[j][s][b * P + u] (op) = x[clamp(S * j + (b - L) * D, 0, len_s - 1)][s][u] (op), bits copied; zeros
//                          on the rows j >= n_s (no real frames) and in pad columns
//   context_bwd_kernel     dx[ts][s][u] (fp32) = the sum of e[j][s][b * P + u] over the (b, j) that read parent frame ts, b
//                          ascending, then j ascending, single fp32 additions from +0.0f; +0.0 for a frame nobody reads; zeros
//                          on every other row of the parent's fraction and in pad columns
// All are streaming kernels: grid-stride loops, no LDS, no atomics.  The context layer's rows are dense (unit u of block b at
// column b * P + u); the predecessor's may be split (a blstm), which its map (cn_unit_map.h) translates.  The gather and the fold
// take S as a compile-time 1 for the plain layer (STRIDED = false), whose code so has no multiplication or division by it.
//
// Thread map of the gather and the fold, as in cn_splice.hip: a thread owns VEC neighbouring columns of one row and stores them
// as one 16-byte piece (the gather: 4 fp32 / 8 bf16 operands of a context row; the fold: 4 fp32 of a predecessor row),
// neighbouring threads own neighbouring pieces, so a wave stores one contiguous KiB and loads runs of contiguous units of one
// source row.  Where P and a split predecessor's H are multiples of VEC a piece lies in one block and one direction and its source
// starts on 16 bytes: it is loaded as one piece too (RUN).  Otherwise (the headline's H = 125) the piece is put together from
// element loads, which neighbouring lanes still take from neighbouring addresses: the scalar path, which also serves a source
// that does not start on 16 bytes.  The stores are always whole pieces: both kernels write buffers of this library's own
// allocation whose rows are multiples of 32 elements (cn_layer_create*).  At the sizes of a fraction both buffers stay in the
// L2 / MALL.
#include <type_traits>

#include "cn_internal.h"

namespace cn {

// one wave per slot: lane i counts the frames t = i, i + 64, ..., the lanes' counts are added across the wave
__global__ __launch_bounds__(64) void context_len_kernel(const char *__restrict__ pat, int T, int PSp, int *__restrict__ len)
{
    const int s = blockIdx.x;
    int n = 0;
    for (int t = threadIdx.x; t < T; t += 64) n += pat[(long)t * PSp + s] != 0;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d, 64);
    if (threadIdx.x == 0) len[s] = n;
}

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
__device__ __forceinline__ int context_src(const ContextArgs &a, int S, int j, int b, int len) { return max(0, min(S * j + (b - a.left) * a.dil, len - 1)); }

template <bool F32, int VEC, bool RUN, bool STRIDED>
__global__ __launch_bounds__(256) void context_fwd_kernel(ContextArgs a, const int *__restrict__ len, const void *__restrict__ x, void *__restrict__ out)
{
    typedef typename std::conditional<F32, unsigned, unsigned short>::type op_t;      // (the bits of an operand: nothing is rounded)
    static_assert(VEC * sizeof(op_t) == 16, "a piece is 16 bytes");
    const int S = STRIDED ? a.S : 1;
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    const int pieces = a.Lp / VEC, width = a.B * a.prev.L;
    const long total = (long)a.Tout * a.PSp * pieces;
    for (long idx = tid; idx < total; idx += nth) {
        const long n = idx / pieces; const int c0 = (int)(idx % pieces) * VEC;
        const int j = (int)(n / a.PSp), s = (int)(n % a.PSp);
        const int ln = len[s];
        // (j < n_s = ceil(len_s / S); no holes: the real frames of a slot are 0 .. len - 1; S * j < Tin + S, an int as in context_src)
        const bool live = S * j < ln && c0 < width;
        int b = 0, u = 0;                                  // block and unit of the piece's first column
        if (live) { b = c0 / a.prev.L; u = c0 - b * a.prev.L; }
        if constexpr (RUN) {
            uint4 o = make_uint4(0u, 0u, 0u, 0u);
            if (live) o = *(const uint4 *)((const op_t *)x + ((long)context_src(a, S, j, b, ln) * a.PSp + s) * a.prev.Lp + a.prev.col(u));
            *(uint4 *)((op_t *)out + n * a.Lp + c0) = o;
        } else {
            union { op_t e[VEC]; uint4 q; } v;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                op_t w = 0;
                if (live && c0 + i < width) {
                    w = ((const op_t *)x)[((long)context_src(a, S, j, b, ln) * a.PSp + s) * a.prev.Lp + a.prev.col(u)];
                    if (++u == a.prev.L) { u = 0; ++b; }
                }
                v.e[i] = w;
            }
            *(uint4 *)((op_t *)out + n * a.Lp + c0) = v.q;
        }
    }
}

template <bool RUN, bool STRIDED>
__global__ __launch_bounds__(256) void context_bwd_kernel(ContextArgs a, const int *__restrict__ len, const float *__restrict__ e, float *__restrict__ dx)
{
    constexpr int VEC = 4;                                  // a piece is four fp32
    const int S = STRIDED ? a.S : 1;
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    const int pieces = a.prev.Lp / VEC;
    const long total = (long)a.Tin * a.PSp * pieces;
    for (long idx = tid; idx < total; idx += nth) {
        const long n = idx / pieces; const int c0 = (int)(idx % pieces) * VEC;
        const int t = (int)(n / a.PSp), s = (int)(n % a.PSp);
        const int ln = len[s];
        const int nj = (ln + S - 1) / S;                    // n_s
        // the units of the piece's columns: consecutive from u0, the first cnt columns (cn_unit_map.h); RUN: all four or none
        const int u0 = a.prev.unit(c0);
        const int cnt = a.prev.units_in_group(c0, VEC);
        float acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
        if (t < ln && cnt > 0) {
            for (int b = 0; b < a.B; ++b) {
                // the frames j < n_s with clamp(S * j + o, 0, len - 1) == t: inside the sequence the one j with S * j == t - o,
                // if S divides it; the runs that the clamp folds onto the first and the last frame  (jlo: the quotient of a
                // d <= 0 is <= 0 too)
                const int o = (b - a.left) * a.dil, d = t - o;
                const int jlo = max(t == 0 ? 0 : (d + S - 1) / S, 0);
                const int jhi = t == ln - 1 ? nj - 1 : (d < 0 ? -1 : min(d / S, nj - 1));
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

static int context_blocks(long work) { long b = (work + 255) / 256; return (int)(b > 2048 ? 2048 : b < 1 ? 1 : b); }
// is every piece of `vec` elements one run: every block of P units and every direction of a split predecessor a whole number of them
static bool context_runs(const ContextArgs &a, int vec) { return a.prev.L % vec == 0 && a.prev.H % vec == 0; }
// f(std::true_type or std::false_type) for the run-time v: how the launchers below turn their choices into template arguments
template <class Fn> static void with_bool(bool v, Fn f) { if (v) f(std::true_type{}); else f(std::false_type{}); }

void launch_context_lengths(hipStream_t s, const char *pat, int T, int PSp, int *len)
{
    if (PSp <= 0) return;
    hipLaunchKernelGGL(context_len_kernel, dim3(PSp), dim3(64), 0, s, pat, T, PSp, len);
}

void launch_stride_axis(hipStream_t s, int S, int Tout, int PSp, const int *len, const int *tcls, int *nlen, char *npat, int *ntcls)
{
    if ((long)Tout * PSp <= 0) return;
    hipLaunchKernelGGL(stride_axis_kernel, dim3(context_blocks((long)Tout * PSp)), dim3(256), 0, s, S, Tout, PSp, len, tcls, nlen, npat, ntcls);
}

void launch_stride_targets(hipStream_t s, int rate, int Tout, int PSp, int W, const int *nlen, const float *src, float *tgt)
{
    const long total = (long)Tout * PSp * W; if (total <= 0) return;
    hipLaunchKernelGGL(stride_targets_kernel, dim3(context_blocks(total)), dim3(256), 0, s, rate, Tout, PSp, W, nlen, src, tgt);
}

void launch_context_fwd(hipStream_t s, bool f32, const ContextArgs &a, const int *len, const void *x, void *out)
{
    const long rows = (long)a.Tout * a.PSp; if (rows <= 0) return;
    const int vec = f32 ? 4 : 8;
    const bool runs = context_runs(a, vec) && ((size_t)x & 15) == 0;
    const int blocks = context_blocks(rows * (a.Lp / vec));
    with_bool(f32, [&](auto F32) { with_bool(runs, [&](auto RUN) { with_bool(a.S > 1, [&](auto STRIDED) {
        hipLaunchKernelGGL((context_fwd_kernel<decltype(F32)::value, decltype(F32)::value ? 4 : 8, decltype(RUN)::value, decltype(STRIDED)::value>),
                           dim3(blocks), dim3(256), 0, s, a, len, x, out);
    }); }); });
}

void launch_context_bwd(hipStream_t s, const ContextArgs &a, const int *len, const float *e, float *dx)
{
    const long rows = (long)a.Tin * a.PSp; if (rows <= 0) return;
    const bool runs = context_runs(a, 4) && ((size_t)e & 15) == 0;
    const int blocks = context_blocks(rows * (a.prev.Lp / 4));
    with_bool(runs, [&](auto RUN) { with_bool(a.S > 1, [&](auto STRIDED) {
        hipLaunchKernelGGL((context_bwd_kernel<decltype(RUN)::value, decltype(STRIDED)::value>), dim3(blocks), dim3(256), 0, s, a, len, e, dx);
    }); });
}

}  // namespace cn
