// LAMB (include/currennt_hip.h, section LAMB; no counterpart in the reference): Adam's moments, a direction u per weight, and one
// trust ratio per layer from the norms of the layer's weights and of its direction.  gfx950 only.
//
//   lamb_direction_kernel   m, v, u of every entry; Sw = sum w^2 and Su = sum u^2 per layer in the order of the Gradient clipping
//                           section; the last workgroup to arrive for a layer writes the layer's record {nw, nu, ratio}
//   lamb_apply_kernel       w = w - (lr_layer * ratio) * u
// One launch of each covers every layer of a group: blockIdx.y is the layer, blockIdx.x the part of it.  A layer's range starts on
// a multiple of four floats and its padded count is one (16-byte loads; pad entries are zero and stay zero).
#include "cn_internal.h"

namespace cn {

typedef __attribute__((ext_vector_type(4))) float f32x4;

// The direction of one entry, operation by operation as the header states it.  The plain operators under contract(off), as the
// steps of cn_elementwise.hip and for the reason stated there: the pragma is what keeps a product out of the sum that reads it
// (hipcc's __f*_rn are the plain operators and promise nothing); sqrtf is the correctly rounded sequence, see adam_step.
template <bool DEC>
__device__ __forceinline__ float lamb_direction(float w, float g, float &m, float &v, const LambScalars &a)
{
#pragma clang fp contract(off)
    const float m1 = a.b1 * m, m2 = a.omb1 * g;
    const float mn = m1 + m2;
    const float gg = g * g;
    const float v1 = a.b2 * v, v2 = a.omb2 * gg;
    const float vn = v1 + v2;
    m = mn; v = vn;
    const float num = a.c_t * mn;
    const float den = sqrtf(vn) + a.eps_t;
    const float r = __fdiv_rn(num, den);
    if (!DEC) return r;
    const float dw = a.decay * w;
    return r + dw;
}
__device__ __forceinline__ bool lamb_decays(const LambItem &it, unsigned i) { return i < it.a1 || (i >= it.b0 && i < it.b1); }

// Workgroup (k, layer) owns lanes 1024k .. 1024k + 1023 of the layer's CLIP_LANES lanes, thread t of it lanes 4t .. 4t + 3 of
// those: one 16-byte load per array and row of CLIP_LANES entries, LAMB_UNROLL rows' loads in flight in front of the dependent
// adds (a lane's add chain is the order; the loads are not part of it).  Squares are exact in double, so the fused multiply-add
// rounds what a separate add would.  Rows behind the layer's end add nothing (+0 changes no sum of squares).
// Cross-workgroup part as in grad_norm_kernel: the partials are stored at agent scope and drained in front of the layer's
// counter; the last arriver acquires, adds the CLIP_WGS partials of each sum over neighbours and writes the record.
// clip (nullable): the step's clipping record -- CLIP_SKIP touches nothing, the layer's record included.
__global__ __launch_bounds__(256) void lamb_direction_kernel(LambGroup grp, float *__restrict__ arena, size_t total, float *__restrict__ vbase,
                                                             float *__restrict__ ubase, LambScalars a, LambRecord *recs, const ClipRecord *clip)
{
    int state = CLIP_NONE; float scale = 1.0f;
    if (clip) { state = clip->state; scale = clip->scale; if (state == CLIP_SKIP) return; }
    const LambItem it = grp.item[blockIdx.y];
    float *w = arena + it.off, *m = w + 2 * total, *v = vbase + it.off, *u = ubase + it.off;
    const float *g = w + total;
    const bool decay_on = a.decay != 0.f;
    const unsigned n = it.n;
    double aw0 = 0.0, aw1 = 0.0, aw2 = 0.0, aw3 = 0.0, au0 = 0.0, au1 = 0.0, au2 = 0.0, au3 = 0.0;
    for (unsigned base = 4 * (blockIdx.x * 256 + threadIdx.x); base < n; base += LAMB_UNROLL * CLIP_LANES) {
        f32x4 xw[LAMB_UNROLL], xg[LAMB_UNROLL], xm[LAMB_UNROLL], xv[LAMB_UNROLL];
#pragma unroll
        for (int r = 0; r < LAMB_UNROLL; ++r) {
            const unsigned i = base + (unsigned)r * CLIP_LANES;        // (n is a multiple of 4: a group of four is inside or outside)
            if (i < n) { xw[r] = *(const f32x4 *)(w + i); xg[r] = *(const f32x4 *)(g + i); xm[r] = *(const f32x4 *)(m + i); xv[r] = *(const f32x4 *)(v + i); }
        }
#pragma unroll
        for (int r = 0; r < LAMB_UNROLL; ++r) {
            const unsigned i = base + (unsigned)r * CLIP_LANES;
            if (i >= n) break;
            f32x4 xu;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float ge = xg[r][e], me = xm[r][e], ve = xv[r][e];
                if (state == CLIP_SCALE) ge = __fmul_rn(scale, ge);
                xu[e] = (decay_on && lamb_decays(it, i + e)) ? lamb_direction<true>(xw[r][e], ge, me, ve, a)
                                                             : lamb_direction<false>(xw[r][e], ge, me, ve, a);
                xm[r][e] = me; xv[r][e] = ve;
            }
            *(f32x4 *)(m + i) = xm[r]; *(f32x4 *)(v + i) = xv[r]; *(f32x4 *)(u + i) = xu;
            const double w0 = xw[r][0], w1 = xw[r][1], w2 = xw[r][2], w3 = xw[r][3];
            const double u0 = xu[0], u1 = xu[1], u2 = xu[2], u3 = xu[3];
            aw0 = __fma_rn(w0, w0, aw0); aw1 = __fma_rn(w1, w1, aw1); aw2 = __fma_rn(w2, w2, aw2); aw3 = __fma_rn(w3, w3, aw3);
            au0 = __fma_rn(u0, u0, au0); au1 = __fma_rn(u1, u1, au1); au2 = __fma_rn(u2, u2, au2); au3 = __fma_rn(u3, u3, au3);
        }
    }
    __shared__ double shw[256], shu[256];
    shw[threadIdx.x] = __dadd_rn(__dadd_rn(aw0, aw1), __dadd_rn(aw2, aw3));
    shu[threadIdx.x] = __dadd_rn(__dadd_rn(au0, au1), __dadd_rn(au2, au3));
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {             // level by level over neighbours: s results, result t = pair (2t, 2t + 1)
        double x = 0.0, y = 0.0;
        if (threadIdx.x < s) { x = __dadd_rn(shw[2 * threadIdx.x], shw[2 * threadIdx.x + 1]); y = __dadd_rn(shu[2 * threadIdx.x], shu[2 * threadIdx.x + 1]); }
        __syncthreads();
        if (threadIdx.x < s) { shw[threadIdx.x] = x; shu[threadIdx.x] = y; }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    LambRecord *rec = recs + it.rec;
    __hip_atomic_store(&rec->part_w[blockIdx.x], shw[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&rec->part_u[blockIdx.x], shu[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // (the partials must have arrived before this workgroup is counted: see rowstat_reduce_wave)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (__hip_atomic_fetch_add(&rec->arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != CLIP_WGS - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double pw[CLIP_WGS], pu[CLIP_WGS];
#pragma unroll
    for (int k = 0; k < CLIP_WGS; ++k) {
        pw[k] = __hip_atomic_load(&rec->part_w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pu[k] = __hip_atomic_load(&rec->part_u[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int s = CLIP_WGS / 2; s > 0; s >>= 1)
#pragma unroll
        for (int k = 0; k < s; ++k) { pw[k] = __dadd_rn(pw[2 * k], pw[2 * k + 1]); pu[k] = __dadd_rn(pu[2 * k], pu[2 * k + 1]); }
    const double Sw = pw[0], Su = pu[0];
    const float nw = (float)__dsqrt_rn(Sw), nu = (float)__dsqrt_rn(Su);          // correctly rounded in double, rounded once to float
    float ratio = 1.0f;
    if (Sw <= 1.7976931348623157e308 && Su <= 1.7976931348623157e308 && nw != 0.f && nu != 0.f) {
        ratio = __fdiv_rn(nw, nu);
        if (ratio < a.min_ratio) ratio = a.min_ratio;
        if (a.max_ratio != 0.f && ratio > a.max_ratio) ratio = a.max_ratio;
    }
    rec->nw = nw; rec->nu = nu; rec->ratio = ratio;
    __hip_atomic_store(&rec->arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (zero again for the next launch)
}

__device__ __forceinline__ float lamb_apply(float w, float step, float u)
{
#pragma clang fp contract(off)
    const float d = step * u;
    return w - d;
}
// behind lamb_direction_kernel on the same stream: a grid-stride loop of 16-byte pieces over each layer's range
__global__ __launch_bounds__(256) void lamb_apply_kernel(LambGroup grp, float *__restrict__ arena, const float *__restrict__ ubase,
                                                         const LambRecord *__restrict__ recs, const ClipRecord *clip)
{
    if (clip && clip->state == CLIP_SKIP) return;
    const LambItem it = grp.item[blockIdx.y];
    const float step = __fmul_rn(it.lr, recs[it.rec].ratio);
    f32x4 *w = (f32x4 *)(arena + it.off);
    const f32x4 *u = (const f32x4 *)(ubase + it.off);
    const unsigned n4 = it.n >> 2, nth = gridDim.x * 256;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n4; i += nth) {
        f32x4 x = w[i];
        const f32x4 d = u[i];
        x[0] = lamb_apply(x[0], step, d[0]); x[1] = lamb_apply(x[1], step, d[1]);
        x[2] = lamb_apply(x[2], step, d[2]); x[3] = lamb_apply(x[3], step, d[3]);
        w[i] = x;
    }
}

void launch_lamb(hipStream_t s, const LambGroup &grp, float *arena, size_t total, float *v, float *u, const LambScalars &a, LambRecord *recs,
                 const ClipRecord *clip, hipEvent_t done)
{
    if (grp.n == 0) return;
    unsigned nmax = 0;
    for (int i = 0; i < grp.n; ++i) nmax = grp.item[i].n > nmax ? grp.item[i].n : nmax;
    hipLaunchKernelGGL(lamb_direction_kernel, dim3(CLIP_WGS, grp.n), dim3(256), 0, s, grp, arena, total, v, u, a, recs, clip);
    unsigned blocks = (nmax / 4 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > LAMB_APPLY_MAX_BLOCKS) blocks = LAMB_APPLY_MAX_BLOCKS;
    hipExtLaunchKernelGGL(lamb_apply_kernel, dim3(blocks, grp.n), dim3(256), 0, s, nullptr, done, 0, grp, arena, (const float *)u, (const LambRecord *)recs, clip);
}

}  // namespace cn
