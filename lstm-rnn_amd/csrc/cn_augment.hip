// Input augmentation on the device (include/currennt_hip.h, section Input augmentation): Gaussian input noise
// (--input_noise_sigma, DataSet.cpp:177-184 of the reference, drawn there on the loader thread) and SpecAugment's frequency and
// time masks (Park et al. 2019; no counterpart in the reference), applied where a fraction is re-laid out.  gfx950 only.
//
//   augment_table_kernel          per slot: the sequence's length and its mask intervals          (one small workgroup)
//   fraction_load_augment_kernel  fraction_load_kernel of cn_elementwise.hip + the augmentation   (resident and staged loads)
//   pad_convert_augment_kernel    pad_convert_kernel + the augmentation                           (option overlap = 0)
// Both re-layouts call augment_value (cn_augment_device.h), the one statement of the per-element arithmetic.
#include "cn_internal.h"
#include "cn_philox_device.h"
#include "cn_augment_device.h"

namespace cn {

// (as in cn_elementwise.hip)
template <bool F32> __device__ __forceinline__ void st_op(void *base, long idx, float v)
{
    if constexpr (F32) ((float *)base)[idx] = v; else ((__bf16 *)base)[idx] = (__bf16)v;      // (bf16: round to nearest even)
}

// One thread per slot: len_s = frames whose pattern type is not NONE, then mask m's (start, width) from
// Philox(counter = (m, s, pass), key "mask"): frequency mask i is m = i, time mask i is m = 16 + i.  A slot with len_s = 0 gets
// zeros: the re-layout copies it unchanged.
__global__ __launch_bounds__(256) void augment_table_kernel(AugArgs a, const char *__restrict__ pat, int pstride, int T, int PS, int *__restrict__ tab)
{
    for (int s = threadIdx.x; s < PS; s += blockDim.x) {
        int len = 0;
        for (int t = 0; t < T; ++t) len += pat[(long)t * pstride + s] != 0;
        int *row = tab + (long)s * AUG_TAB_STRIDE;
        row[0] = len;
#pragma unroll 1
        for (int i = 0; i < 2 * AUG_MAX_MASKS; ++i) {
            const bool time = i >= AUG_MAX_MASKS;
            const int k = time ? i - AUG_MAX_MASKS : i;
            int start = 0, width = 0;
            if (len >= 1 && k < (time ? a.ntime : a.nfreq)) {
                const uint4 w = philox4x32_10(make_uint4((uint32_t)(time ? 16 + k : k), (uint32_t)s, a.pass_lo, a.pass_hi), a.k0, a.k1_mask);
                const int range = time ? len : a.P0;                                              // what the mask lies in: [0, range)
                const int cap = time ? min(a.twidth, (int)((long)len * a.permille / 1000)) : min(a.fwidth, a.P0);
                width = (int)(w.x % (uint32_t)(cap + 1));                                          // (modulo bias <= 2^-32 * range: ignored)
                start = (int)(w.y % (uint32_t)(range - width + 1));
            }
            row[1 + 2 * i] = start; row[2 + 2 * i] = width;
        }
    }
}

// Everything fraction_load_kernel does; the input loop augments the real frames on the way.
template <bool F32>
__global__ void fraction_load_augment_kernel(AugArgs a, const int *__restrict__ tab, int T, int PS, int PSp, const char *pat, char *dpat,
                                             const int *tcls, int *dtcls, const float *tgt, float *dtgt, int W, const float *in, int P, void *dst, int Pp)
{
    const long N = (long)T * PSp;
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    for (long n = tid; n < N; n += nth) {
        const long t = n / PSp; const int sl = n % PSp;
        const bool real = sl < PS;
        dpat[n] = real ? pat[t * PS + sl] : 0;
        if (tcls) dtcls[n] = real ? tcls[t * PS + sl] : -1;
    }
    if (tgt)
        for (long idx = tid; idx < N * W; idx += nth) {
            const long n = idx / W; const int j = idx % W;
            const long t = n / PSp; const int sl = n % PSp;
            dtgt[idx] = sl < PS ? tgt[(t * PS + sl) * W + j] : 0.f;
        }
    for (long idx = tid; idx < N * Pp; idx += nth) {
        const long n = idx / Pp; const int c = idx % Pp;
        const long t = n / PSp; const int sl = n % PSp;
        float v = 0.f;
        if (sl < PS && c < P) {
            v = in[(t * PS + sl) * P + c];
            if (pat[t * PS + sl] != 0) v = augment_value(a, tab + (long)sl * AUG_TAB_STRIDE, sl, (int)t, c, v);
        }
        st_op<F32>(dst, idx, v);
    }
}

// pad_convert_kernel on inputs that are already in the device's row layout (row n = t * PSp + sl), augmented on the way
template <bool F32>
__global__ void pad_convert_augment_kernel(AugArgs a, const int *__restrict__ tab, const float *src, const char *dpat, int T, int PS, int PSp,
                                           int P, void *dst, int Pp)
{
    const long total = (long)T * PSp * Pp;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long n = idx / Pp; const int c = idx % Pp;
        const long t = n / PSp; const int sl = n % PSp;
        float v = 0.f;
        if (c < P) {
            v = src[n * P + c];
            if (sl < PS && dpat[n] != 0) v = augment_value(a, tab + (long)sl * AUG_TAB_STRIDE, sl, (int)t, c, v);
        }
        st_op<F32>(dst, idx, v);
    }
}

void launch_augment_table(hipStream_t s, const AugArgs &a, const char *pat, int pstride, int T, int PS, int *tab)
{
    if (PS <= 0 || T <= 0) return;
    hipLaunchKernelGGL(augment_table_kernel, dim3(1), dim3(PS <= 64 ? 64 : 256), 0, s, a, pat, pstride, T, PS, tab);
}
void launch_fraction_load_augment(hipStream_t s, bool f32, const AugArgs &a, const int *tab, int T, int PS, int PSp, const char *pat, char *dpat,
                                  const int *tcls, int *dtcls, const float *tgt, float *dtgt, int W, const float *in, int P, void *dst, int Pp,
                                  int *rm, int maxN, int Tmin)
{
    long total = (long)T * PSp * Pp; if (total <= 0) return;
    int blocks = (int)((total + 255) / 256); if (blocks > 2048) blocks = 2048;
    if (f32) hipLaunchKernelGGL(fraction_load_augment_kernel<true>, dim3(blocks), dim3(256), 0, s, a, tab, T, PS, PSp, pat, dpat, tcls, dtcls, tgt, dtgt, W, in, P, dst, Pp);
    else     hipLaunchKernelGGL(fraction_load_augment_kernel<false>, dim3(blocks), dim3(256), 0, s, a, tab, T, PS, PSp, pat, dpat, tcls, dtcls, tgt, dtgt, W, in, P, dst, Pp);
    launch_rowmap(s, dpat, T * PSp, rm, maxN, Tmin * PSp);
}
void launch_pad_convert_augment(hipStream_t s, bool f32, const AugArgs &a, const int *tab, const float *src, const char *dpat, int T, int PS, int PSp,
                                int P, void *dst, int Pp)
{
    long total = (long)T * PSp * Pp; if (total <= 0) return;
    int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096;
    if (f32) hipLaunchKernelGGL(pad_convert_augment_kernel<true>, dim3(blocks), dim3(256), 0, s, a, tab, src, dpat, T, PS, PSp, P, dst, Pp);
    else     hipLaunchKernelGGL(pad_convert_augment_kernel<false>, dim3(blocks), dim3(256), 0, s, a, tab, src, dpat, T, PS, PSp, P, dst, Pp);
}

}  // namespace cn
