// Input splicing and frame skipping on the device (include/currennt_hip.h, section of that name; no counterpart in the
// reference, which splices on the host and never skips).  gfx950 only.
//
//   fraction_load_splice_kernel   a SOURCE-rate fraction of unspliced patterns -> the network-rate fraction in the device layout:
//                                 derived pattern types, classes / target rows of source row K * j, the gathered inputs (through
//                                 augment_value of cn_augment_device.h when the load augments)
// In front of it launch_augment_table (cn_augment.hip) forms len_s per slot from the source pattern types; behind it launch_rowmap.
//
// Thread map of the gather: a thread owns VEC neighbouring columns of one network row and stores them as one 16-byte piece
// (VEC = 4 fp32 / 8 bf16 operands; Pp is a multiple of 32, so a piece never straddles a row), neighbouring threads own
// neighbouring pieces: a wave's stores are one contiguous KiB, and its loads are runs of P0 contiguous floats of one source row
// (block b of network frame j reads source frame clamp(K * j + b - L)), a few rows per wave.  The source is read B / K times on
// average; at the sizes of a fraction (a few MB) it stays in the L2 / MALL.
#include "cn_internal.h"
#include "cn_augment_device.h"

namespace cn {

// pattern types as DataSet.hpp / fraction.py number them
enum { SPL_NONE = 0, SPL_FIRST = 1, SPL_NORMAL = 2, SPL_LAST = 3 };

// VEC operands of one row as one store (VEC * sizeof(operand) = 16 bytes), or a single one
template <bool F32, int VEC> __device__ __forceinline__ void st_piece(void *base, long idx, const float *v)
{
    if constexpr (VEC == 1) {
        if constexpr (F32) ((float *)base)[idx] = v[0]; else ((__bf16 *)base)[idx] = (__bf16)v[0];      // (bf16: round to nearest even)
    } else if constexpr (F32) {
        static_assert(VEC == 4, "a 16-byte piece is four fp32 operands");
        *(float4 *)((float *)base + idx) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        static_assert(VEC == 8, "a 16-byte piece is eight bf16 operands");
        union { __bf16 h[8]; uint4 q; } u;
#pragma unroll
        for (int i = 0; i < 8; ++i) u.h[i] = (__bf16)v[i];
        *(uint4 *)((__bf16 *)base + idx) = u.q;
    }
}

// Network row n = j * PSp + sl (j < Tnet).  Slot sl < PS with len = tab[sl][0] source frames owns n_s = ceil(len / K) network
// frames; everything else is a dummy row: NONE, class -1, zero targets, zero inputs.  Nothing is read from the source beyond
// frame len - 1 of a slot, and len <= Tsrc by construction of the table.
template <bool F32, int VEC, bool AUG>
__global__ __launch_bounds__(256) void fraction_load_splice_kernel(AugArgs a, const int *__restrict__ tab, int Tnet, int PS, int PSp, char *dpat,
                                                                   const int *tcls, int *dtcls, const float *tgt, float *dtgt, int W,
                                                                   const float *__restrict__ in, int P, void *dst, int Pp)
{
    const long N = (long)Tnet * PSp;
    const int K = a.skip, P0 = a.P0;
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    for (long n = tid; n < N; n += nth) {
        const int j = (int)(n / PSp), sl = (int)(n % PSp);
        const int ns = sl < PS ? (tab[(long)sl * AUG_TAB_STRIDE] + K - 1) / K : 0;
        const bool real = j < ns;
        dpat[n] = !real ? SPL_NONE : j == 0 ? SPL_FIRST : j == ns - 1 ? SPL_LAST : SPL_NORMAL;
        if (tcls) dtcls[n] = real ? tcls[(long)K * j * PS + sl] : -1;
    }
    if (tgt)
        for (long idx = tid; idx < N * W; idx += nth) {
            const long n = idx / W; const int w = (int)(idx % W);
            const int j = (int)(n / PSp), sl = (int)(n % PSp);
            const int ns = sl < PS ? (tab[(long)sl * AUG_TAB_STRIDE] + K - 1) / K : 0;
            dtgt[idx] = j < ns ? tgt[((long)K * j * PS + sl) * W + w] : 0.f;
        }
    const int pieces = Pp / VEC;
    for (long idx = tid; idx < N * pieces; idx += nth) {
        const long n = idx / pieces; const int c0 = (int)(idx % pieces) * VEC;
        const int j = (int)(n / PSp), sl = (int)(n % PSp);
        const int *row = tab + (long)sl * AUG_TAB_STRIDE;
        const int len = sl < PS ? row[0] : 0;
        const bool real = j < (len + K - 1) / K;
        float v[VEC];
        int b = c0 / P0, f = c0 - b * P0;                              // block and feature of the piece's first column, stepped below
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const int c = c0 + i;
            float x = 0.f;
            if (real && c < P) {
                const int ts = max(0, min(K * j + b - a.ctx_left, len - 1));
                x = in[((long)ts * PS + sl) * P0 + f];
                if constexpr (AUG) x = augment_value(a, row, sl, j, c, x);
            }
            v[i] = x;
            if (++f == P0) { f = 0; ++b; }
        }
        st_piece<F32, VEC>(dst, n * Pp + c0, v);
    }
}

template <bool F32, int VEC>
static void launch_splice_kernel(hipStream_t s, int blocks, bool augment, const AugArgs &a, const int *tab, int Tnet, int PS, int PSp, char *dpat,
                                 const int *tcls, int *dtcls, const float *tgt, float *dtgt, int W, const float *in, int P, void *dst, int Pp)
{
    if (augment) hipLaunchKernelGGL((fraction_load_splice_kernel<F32, VEC, true>), dim3(blocks), dim3(256), 0, s, a, tab, Tnet, PS, PSp, dpat, tcls, dtcls, tgt, dtgt, W, in, P, dst, Pp);
    else         hipLaunchKernelGGL((fraction_load_splice_kernel<F32, VEC, false>), dim3(blocks), dim3(256), 0, s, a, tab, Tnet, PS, PSp, dpat, tcls, dtcls, tgt, dtgt, W, in, P, dst, Pp);
}

void launch_fraction_load_splice(hipStream_t s, bool f32, const AugArgs &a, bool augment, const int *tab, int Tnet, int PS, int PSp,
                                 char *dpat, const int *tcls, int *dtcls, const float *tgt, float *dtgt, int W, const float *in, int P,
                                 void *dst, int Pp, int *rm, int maxN, int Tmin_net)
{
    const int vec = f32 ? 4 : 8;
    const bool wide = Pp % vec == 0 && ((size_t)dst & 15) == 0;      // whole 16-byte pieces per row, rows that start on one
    long total = (long)Tnet * PSp * (wide ? Pp / vec : Pp); if (total <= 0) return;
    int blocks = (int)((total + 255) / 256); if (blocks > 2048) blocks = 2048;
    if (f32) {
        if (wide) launch_splice_kernel<true, 4>(s, blocks, augment, a, tab, Tnet, PS, PSp, dpat, tcls, dtcls, tgt, dtgt, W, in, P, dst, Pp);
        else      launch_splice_kernel<true, 1>(s, blocks, augment, a, tab, Tnet, PS, PSp, dpat, tcls, dtcls, tgt, dtgt, W, in, P, dst, Pp);
    } else {
        if (wide) launch_splice_kernel<false, 8>(s, blocks, augment, a, tab, Tnet, PS, PSp, dpat, tcls, dtcls, tgt, dtgt, W, in, P, dst, Pp);
        else      launch_splice_kernel<false, 1>(s, blocks, augment, a, tab, Tnet, PS, PSp, dpat, tcls, dtcls, tgt, dtgt, W, in, P, dst, Pp);
    }
    launch_rowmap(s, dpat, Tnet * PSp, rm, maxN, Tmin_net * PSp);
}

}  // namespace cn
