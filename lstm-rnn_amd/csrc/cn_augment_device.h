// The per-element arithmetic of the input augmentation (include/currennt_hip.h, section Input augmentation), shared by the
// re-layouts of cn_augment.hip and the spliced re-layout of cn_splice.hip: the one statement of it.
#pragma once

#include "cn_internal.h"
#include "cn_philox_device.h"

namespace cn {

// x' of input element (slot s, time t, column c) of a frame whose pattern type is not NONE; `row` is the slot's table entry.
// The noise and the masks are functions of the SOURCE element (s, ts, j): every context copy of a frame carries the same ones.
// t counts network frames: frame t is centred on source frame a.skip * t (a.skip = 1: the caller spliced, t is the source frame).
// (One Philox call per element: sharing a call among the four elements of a group would need a thread to own four source
// elements, which a context copy's column order does not give; the call is ~60 integer instructions on a bandwidth-bound launch.)
__device__ __forceinline__ float augment_value(const AugArgs &a, const int *__restrict__ row, int s, int t, int c, float x)
{
    const int len = row[0];
    const int b = c / a.P0, j = c - b * a.P0;
    const int ts = max(0, min(a.skip * t + b - a.ctx_left, len - 1));
    bool masked = false;
    for (int m = 0; m < a.nfreq; ++m) masked |= (unsigned)(j - row[1 + 2 * m]) < (unsigned)row[2 + 2 * m];
    const int *trow = row + 2 * AUG_MAX_MASKS;
    for (int m = 0; m < a.ntime; ++m) masked |= (unsigned)(ts - trow[1 + 2 * m]) < (unsigned)trow[2 + 2 * m];
    if (masked) return 0.f;
    if (a.sigma == 0.f) return x;
    const long e = (long)ts * a.P0 + j;
    const uint4 w = philox4x32_10(make_uint4((uint32_t)(e >> 2), (uint32_t)s, a.pass_lo, a.pass_hi), a.k0, a.k1_noise);
    return __fadd_rn(x, gauss_noise(w, e, a.sigma));
}

}  // namespace cn
