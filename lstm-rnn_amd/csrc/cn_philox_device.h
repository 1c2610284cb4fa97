// Device functions the counter-based random streams share (include/currennt_hip.h, sections Dropout, Weight noise and Input
// augmentation): Philox4x32-10 and the Box-Muller step from four of its words to one Gaussian sample.  Included by
// cn_elementwise.hip (dropout masks, weight noise) and cn_augment.hip (input noise, SpecAugment masks).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cn {

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c;
}

// n = sigma * z of index k from the words w of its group of four (k >> 2): the arithmetic of section Weight noise
__device__ __forceinline__ float gauss_noise(uint4 w, long k, float sigma)
{
    const bool second = (k & 2) != 0;                                          // the pair of this index: words (0, 1) or (2, 3)
    const uint32_t a = second ? w.z : w.x, b = second ? w.w : w.y;
    const float u1 = (float)(2u * (a >> 9) + 1u) * 0x1p-24f;                   // odd multiples of 2^-24 / 2^-23 below 2^24: exact
    const float t = (float)(2u * (b >> 9) + 1u) * 0x1p-23f;
    const float r = sqrtf(__fmul_rn(-2.0f, logf(u1)));                         // (sqrtf: the correctly rounded one, see adam_step)
    const float z = __fmul_rn(r, (k & 1) ? sinpif(t) : cospif(t));
    return __fmul_rn(sigma, z);
}

}  // namespace cn
