// Connectionist Temporal Classification (Graves et al. 2006) as a post output layer behind a softmax layer: the error -log p(l|x)
// of a label sequence l under all its alignments, and dL/dy for the softmax layer's outputErrors.  The reference has no
// counterpart (its post output layers are per frame: LayerFactory.cu:52-87).
//
// One sequence, slot s of the fraction: device rows n = t * PSp + s, len = number of t with pat[n] != 0, labels l[0 .. U), blank =
// the last unit C - 1, extended sequence l' = (b, l0, b, l1, ..., b) with S = 2U + 1 states.
//
// Arithmetic.  All state is fp32.  A probability of the sweeps is a pair (m, k): the value m * 2^k with a float m in [0.5, 1) and an
// int k of its own -- a power-of-two scale PER STATE, so rescaling never rounds and no state is lost however far below the
// column's largest it lies (a scale shared by a column loses, in fp32, every state more than 2^-126 below the sum: with T = 2000
// and U = 300 on random posteriors those are the states every alignment that reaches the end passes through).  Zero is
// (0, KMIN).  The sum of pairs aligns to the largest exponent K: sum = (ldexp(m0, k0 - K) + ldexp(m1, k1 - K)) + ldexp(m2, k2 - K),
// in that order; norm(x, K) = (frexp mantissa of x, K + frexp exponent of x), or zero for x = 0.
//      a_0(s)  = norm(y_0(l'_s), 0) for s < 2, else zero
//      a_t(s)  = norm(y_t(l'_s) * sum, K)      of a_{t-1}(s), a_{t-1}(s-1) and, if l'_s != b and l'_s != l'_{s-2}, a_{t-1}(s-2)
//      (m, K)  = sum of a_{len-1}(S-1) and a_{len-1}(S-2);      -log p = -((float)K * ln 2 + log m)
// has one logarithm and two roundings whatever the length.  The beta sweep (beta_t without y_t) runs the same way from the end:
//      b_{len-1}(s) = (0.5, 1) for s >= S - 2, else zero;       q_t(s) = norm(m * y_t(l'_s), k) for b_t(s) = (m, k)
//      b_t(s) = norm(sum, K)                   of q_{t+1}(s), q_{t+1}(s+1) and, if l'_{s+2} != b and l'_{s+2} != l'_s, q_{t+1}(s+2)
// The state posterior is gamma_t(s) = a_t(s) b_t(s) / sum_s a_t(s) b_t(s), formed as ldexp(m_a m_b, k_a + k_b - Kmax) with Kmax
// the row's largest k_a + k_b, and
//      dL/dy_k(t) = -(sum over s with l'_s = k of gamma_t(s)) / y_k(t)          (0 where the sum is 0, also at y = 0).
//
// Launches.  ctc_sweep_kernel: grid (PSp, 2), one workgroup per sequence and direction, so the alpha and the beta sweep of a
// sequence run concurrently on two CUs.  Thread i owns states i, i + blockDim, ...; the column a step reads lies in LDS as 8-byte
// pairs (two buffers, so a step has ONE barrier and no reduction), neighbours s-1 / s-2 come from there, the gathers y_t(l'_s)
// are issued D steps ahead into a register ring.  Both sweeps store their columns ([slot][t][Sp] pairs each).
// ctc_errors_kernel: one workgroup per row (t, slot), parallel over t: products, their sum in a fixed order, the blank's sum in
// a fixed order, and every other class summed by the thread of its FIRST occurrence in l along the chain of later occurrences
// (built on the host when the labels are set) -- no atomics, so a repeated label accumulates into its class and two runs give the
// same bits.  Every row and every one of the Lp columns is written; rows outside a sequence, empty and pad slots, pad columns and
// classes outside l' get 0.
//
// An infeasible sequence (len = 0, or U + adjacent repeats > len) and one whose p is 0 contribute error 0, count 0 and zero output
// errors.  The error -log p goes to rowstat[slot] with 1 in the second component; rowstat_reduce_kernel sums the PSp pairs in its
// fixed order.
#include "cn_internal.h"

namespace cn {

namespace {

constexpr float LN2 = 0.69314718055994530942f;
constexpr int KMIN = -(1 << 28);          // exponent of zero: below every real one, and two of them still add without overflow

// a pair (m, k) as it lies in LDS and in the workspace
__device__ __forceinline__ int2 pair(float m, int k) { return make_int2(__float_as_int(m), k); }
__device__ __forceinline__ float mant(int2 p) { return __int_as_float(p.x); }
__device__ __forceinline__ int2 norm(float x, int K)
{
    if (!(x > 0.f)) return pair(0.f, KMIN);
    int e;
    const float m = frexpf(x, &e);
    return pair(m, K + e);
}
// sum of three pairs aligned to their largest exponent (*K); `third`: p2 takes part
__device__ __forceinline__ float sum3(int2 p0, int2 p1, int2 p2, bool third, int *K)
{
    int k = p0.y > p1.y ? p0.y : p1.y;
    if (third && p2.y > k) k = p2.y;
    *K = k;
    const float v = ldexpf(mant(p0), p0.y - k) + ldexpf(mant(p1), p1.y - k);
    return third ? v + ldexpf(mant(p2), p2.y - k) : v;
}

__device__ __forceinline__ float wave_sum_f(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_max_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}

// K states per thread, gathers D steps ahead.  Dynamic LDS: two columns of K * blockDim + 6 pairs (two zeros in front, four
// behind: the neighbours of the first and last state).
template <int K, int D>
__global__ __launch_bounds__(256) void ctc_sweep_kernel(CtcArgs a)
{
    extern __shared__ __align__(16) int2 lds2[];
    __shared__ int red[2][4];
    const int slot = blockIdx.x, beta = a.only ? a.only - 1 : blockIdx.y;
    const int tid = threadIdx.x, nth = blockDim.x, nw = nth >> 6, wave = tid >> 6, lane = tid & 63;
    const int colw = K * nth + 6;
    int2 *col[2] = {lds2, lds2 + colw};

    const int U = a.laboff[slot + 1] - a.laboff[slot];
    const int *lab = a.labels + a.laboff[slot];
    const int S = 2 * U + 1;
    // len and the adjacent repeats of l
    int cnt = 0, rep = 0;
    for (int t = tid; t < a.T; t += nth) cnt += a.pat[(long)t * a.PSp + slot] != 0;
    for (int u = 1 + tid; u < U; u += nth) rep += lab[u] == lab[u - 1];
    cnt = wave_sum_i(cnt); rep = wave_sum_i(rep);
    if (lane == 0) { red[0][wave] = cnt; red[1][wave] = rep; }
    for (int i = tid; i < 2 * colw; i += nth) lds2[i] = pair(0.f, KMIN);
    __syncthreads();
    int len = 0; rep = 0;
    for (int w = 0; w < nw; ++w) { len += red[0][w]; rep += red[1][w]; }
    if (len == 0 || U + rep > len) {                  // infeasible: nothing to sweep (workgroup-uniform)
        if (!beta && tid == 0) { a.info[2 * slot] = len; a.info[2 * slot + 1] = 0; ((float2 *)a.rowstat)[slot] = make_float2(0.f, 0.f); }
        return;
    }

    // this thread's states: class, whether the skip transition enters (alpha: from s-2; beta: from s+2), whether the state exists
    int cls[K]; bool skip[K], act[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = tid + k * nth;
        act[k] = s < S;
        cls[k] = (act[k] && (s & 1)) ? lab[s >> 1] : a.C - 1;
        if (!beta) skip[k] = act[k] && (s & 1) && s >= 3 && lab[s >> 1] != lab[(s >> 1) - 1];
        else       skip[k] = (s & 1) && s + 2 < S && lab[(s >> 1) + 1] != lab[s >> 1];
    }
    const float *y = a.y + (long)slot * a.Lp;         // row t: y + t * PSp * Lp
    const long ystep = (long)a.PSp * a.Lp;
    int2 *ws = (beta ? a.beta : a.alpha) + (long)slot * a.T * a.Sp;
    const int t0 = beta ? len - 1 : 0, dt = beta ? -1 : 1;

    // register ring of gathered posteriors: ring[k][j] belongs to step i with i % D == j (steps count from 0 in sweep direction)
    float ring[K][D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        const int i = j < len ? j : len - 1;
#pragma unroll
        for (int k = 0; k < K; ++k) ring[k][j] = y[(long)(t0 + dt * i) * ystep + cls[k]];
    }

    for (int i0 = 0; i0 < len; i0 += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int i = i0 + j;
            if (i < len) {                            // (workgroup-uniform)
                const int t = t0 + dt * i, cur = i & 1, prv = cur ^ 1;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int s = tid + k * nth;
                    const float yv = ring[k][j];
                    int2 v, q;                        // v: what the workspace keeps; q: what the next step reads
                    if (!beta) {
                        if (i == 0) v = (act[k] && s < 2) ? norm(yv, 0) : pair(0.f, KMIN);
                        else {
                            const int2 *p = col[prv] + s;           // p[2] = state s, p[1] = s - 1, p[0] = s - 2
                            int Kx;
                            const float sm = sum3(p[2], p[1], p[0], skip[k], &Kx);
                            v = act[k] ? norm(yv * sm, Kx) : pair(0.f, KMIN);
                        }
                        q = v;
                    } else {
                        if (i == 0) v = (act[k] && s >= S - 2) ? pair(0.5f, 1) : pair(0.f, KMIN);
                        else {
                            const int2 *p = col[prv] + s + 2;       // p[0] = state s, p[1] = s + 1, p[2] = s + 2
                            int Kx;
                            const float sm = sum3(p[0], p[1], p[2], skip[k], &Kx);
                            v = act[k] ? norm(sm, Kx) : pair(0.f, KMIN);
                        }
                        q = norm(mant(v) * yv, v.y);
                    }
                    col[cur][s + 2] = q;
                    if (s < a.Sp) ws[(long)t * a.Sp + s] = v;
                }
                // the gathers of step i + D take this step's place in the ring
                const int in = i + D < len ? i + D : len - 1;
#pragma unroll
                for (int k = 0; k < K; ++k) ring[k][j] = y[(long)(t0 + dt * in) * ystep + cls[k]];
                __syncthreads();
            }
        }
    }
    if (!beta && tid == 0) {
        const int2 *p = col[(len - 1) & 1] + 2;
        int Kx;
        const float fin = sum3(p[S - 1], S > 1 ? p[S - 2] : pair(0.f, KMIN), pair(0.f, KMIN), false, &Kx);
        const bool ok = fin > 0.f;
        a.info[2 * slot] = len; a.info[2 * slot + 1] = ok;
        ((float2 *)a.rowstat)[slot] = ok ? make_float2(-((float)Kx * LN2 + logf(fin)), 1.f) : make_float2(0.f, 0.f);
    }
}

// One workgroup of 128 threads per row.  Dynamic LDS: the row's products [maxS] and their exponents [maxS], the output row [Lp].
__global__ __launch_bounds__(128) void ctc_errors_kernel(CtcArgs a)
{
    extern __shared__ __align__(16) float lds[];
    __shared__ float red[2][2];
    __shared__ int redk[2];
    const int t = blockIdx.x, slot = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float *prod = lds; int *pexp = (int *)(lds + a.maxS); float *row = lds + 2 * a.maxS;
    const long n = (long)t * a.PSp + slot;
    float *er = a.err + n * a.Lp;
    const bool real = a.info[2 * slot + 1] != 0 && t < a.info[2 * slot];     // (pad and empty slots: the sweep found len = 0)
    if (!real) {
        for (int j = tid; j < a.Lp; j += 128) er[j] = 0.f;
        return;
    }
    const int U = a.laboff[slot + 1] - a.laboff[slot], S = 2 * U + 1;
    const int *lab = a.labels + a.laboff[slot], *next = a.next + a.laboff[slot], *first = a.first + a.laboff[slot];
    const int2 *al = a.alpha + ((long)slot * a.T + t) * a.Sp, *be = a.beta + ((long)slot * a.T + t) * a.Sp;
    const float *yr = a.y + n * a.Lp;
    int kmax = 2 * KMIN;
    for (int s = tid; s < S; s += 128) {
        const int2 pa = al[s], pb = be[s];
        const int k = pa.y + pb.y;
        prod[s] = mant(pa) * mant(pb); pexp[s] = k;
        kmax = k > kmax ? k : kmax;
    }
    for (int j = tid; j < a.Lp; j += 128) row[j] = 0.f;
    kmax = wave_max_i(kmax);
    if (lane == 0) redk[wave] = kmax;
    __syncthreads();
    kmax = redk[0] > redk[1] ? redk[0] : redk[1];
    float all = 0.f, blank = 0.f;                     // per thread in ascending s, then a fixed tree
    for (int s = tid; s < S; s += 128) {              // (the entries this thread wrote itself)
        const float p = ldexpf(prod[s], pexp[s] - kmax);
        prod[s] = p; all += p;
        if (!(s & 1)) blank += p;
    }
    all = wave_sum_f(all); blank = wave_sum_f(blank);
    if (lane == 0) { red[0][wave] = all; red[1][wave] = blank; }
    __syncthreads();
    all = red[0][0] + red[0][1]; blank = red[1][0] + red[1][1];
    // y * dL/dy = -sum gamma; a class whose sum is 0 (y = 0 included: a carries the factor y) keeps 0
    if (all > 0.f) {
        if (tid == 0 && blank > 0.f) row[a.C - 1] = -(blank / all) / yr[a.C - 1];
        for (int u = tid; u < U; u += 128) {
            if (!first[u]) continue;
            float g = 0.f;
            for (int v = u; v >= 0; v = next[v]) g += prod[2 * v + 1];
            if (g > 0.f) row[lab[u]] = -(g / all) / yr[lab[u]];
        }
    }
    __syncthreads();
    for (int j = tid; j < a.Lp; j += 128) er[j] = row[j];
}

DeviceOnce g_sweep16_once;
template <int K, int D> void sweep(hipStream_t s, const CtcArgs &a, int threads)
{
    const size_t lds = (size_t)2 * (K * threads + 6) * sizeof(int2);
    if (lds > 64 * 1024 && g_sweep16_once.first())
        (void)hipFuncSetAttribute((const void *)ctc_sweep_kernel<K, D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (!opt().ctc_serial_sweeps) { hipLaunchKernelGGL((ctc_sweep_kernel<K, D>), dim3(a.PSp, 2), dim3(threads), lds, s, a); return; }
    for (int only = 1; only <= 2; ++only) {
        CtcArgs one = a; one.only = only;
        hipLaunchKernelGGL((ctc_sweep_kernel<K, D>), dim3(a.PSp, 1), dim3(threads), lds, s, one);
    }
}

}  // namespace

bool ctc_shape_fits(int max_labels, int Lp)
{
    return 2 * max_labels + 1 <= CTC_MAX_STATES && (size_t)(2 * (2 * max_labels + 1) + Lp) * sizeof(float) <= 60 * 1024;
}

void launch_ctc_sweeps(hipStream_t s, const CtcArgs &a)
{
    if (a.T <= 0 || a.PSp <= 0) return;
    const int S = a.maxS;
    if (S <= 256) sweep<1, 4>(s, a, round_up(S, 64));
    else if (S <= 512) sweep<2, 4>(s, a, 256);
    else if (S <= 1024) sweep<4, 4>(s, a, 256);
    else if (S <= 2048) sweep<8, 2>(s, a, 256);
    else sweep<16, 2>(s, a, 256);
}

void launch_ctc_errors(hipStream_t s, const CtcArgs &a)
{
    if (a.T <= 0 || a.PSp <= 0) return;
    const size_t lds = (size_t)(2 * a.maxS + a.Lp) * sizeof(float);
    hipLaunchKernelGGL(ctc_errors_kernel, dim3(a.T, a.PSp), dim3(128), lds, s, a);
}

}  // namespace cn
