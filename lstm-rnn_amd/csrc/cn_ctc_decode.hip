// Best-path decoding of a CTC layer's posteriors and the label error count, on the device: what the driver's evaluation passes
// print as the label error rate, and what `--ff_output_format ctc_labels` writes.  The reference has no counterpart.
//
// One sequence, slot s of the fraction: device rows n = t * PSp + s, len = number of t with pat[n] != 0 (they are the first len
// steps), blank = the last unit C - 1, labels l[0 .. U) as cn_layer_set_label_sequences uploaded them.
//
// The rule, all of it integer work on the fp32 posteriors the softmax layer holds:
//      k_t     = the index of the largest of y_t[0 .. C); of equal values the LOWEST index (the scan `if (y[k] > y[best]) best = k`
//                from best = 0, numpy.argmax).  Pad columns C .. Lp never take part: a row of exact zeros gives 0.
//      decoded = the k_t of t = 0 .. len - 1 with k_t != C - 1 and (t == 0 or k_t != k_{t-1}), in order; D of them
//      dist    = the Levenshtein distance (unit costs for insertion, deletion and substitution) of decoded to l
// Rows with pat = 0 (behind len, pad slots, empty slots) are not read; their k is -1.
//
// Launches:
//   ctc_argmax_kernel    read-once over the real rows, N x Lp x 4 bytes, 16 bytes per lane.  C <= CTC_ARGMAX_WAVE_C (1024): a wave
//                        per row, four rows per workgroup; above: a workgroup of 256 per row.  Every lane scans its columns in
//                        ascending order with `>`, the reduction carries (value, index) pairs and prefers the lower index of equal
//                        values, so the tie rule holds across lanes and waves.
//   ctc_collapse_kernel  one workgroup of 256 per slot: len, then chunks of 256 frames compacted in order by a ballot scan whose
//                        total carries into the next chunk -> decoded[slot][0 .. D), D.  No bound on T.
//                        Then, same workgroup: the distance by anti-diagonals.  Cell (i, j) of the table, i over the SHORTER of
//                        the two sequences (the distance is symmetric), lies on diagonal i + j at index i; a diagonal reads the two
//                        before it, three of min(D, U) + 1 ints rotate in LDS, one barrier per diagonal, D + U diagonals.
//                        LDS bound: 3 * (min(T, label cap) + 1) ints <= 60 KB, i.e. min(T, label cap) <= CTC_DECODE_MAX_SHORT
//                        (5119); a ctc layer's own cap (2047 labels, CTC_MAX_STATES) lies below it, so no layer that exists can
//                        exceed it.  Beyond it: CN_ERR_SHAPE (ctc_decode_fits), never a truncated table.
//                        With `sums`: thread 0 adds dist and U to two 64-bit integers with integer atomics -- any order of
//                        arrival gives the same numbers.
#include "cn_internal.h"

namespace cn {

namespace {

// the better of two (value, index) pairs under the tie rule
__device__ __forceinline__ void take_better(float &v, int &i, float ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void wave_best(float &v, int &i)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        take_better(v, i, ov, oi);
    }
}
// this lane's columns of a row: groups of four at 4 * (first + k * step), ascending
__device__ __forceinline__ void scan_row(const float *row, int C, int first, int step, float &v, int &i)
{
    v = -INFINITY; i = 0x7fffffff;
    for (int c = 4 * first; c < C; c += 4 * step) {
        const float4 q = *(const float4 *)(row + c);          // (rows are Lp floats, Lp a multiple of 32: inside the row, aligned)
        const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < C && e[j] > v) { v = e[j]; i = c + j; }
    }
}

// WAVE: a wave per row, blockDim = 256 = four rows; else a workgroup per row
template <bool WAVE>
__global__ __launch_bounds__(256) void ctc_argmax_kernel(const float *y, const char *pat, int N, int C, int Lp, int *amax)
{
    __shared__ float rv[4];
    __shared__ int ri[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = WAVE ? blockIdx.x * 4 + wave : blockIdx.x;
    if (n >= N) return;                                       // (wave-uniform; the wave form has no barrier)
    const bool real = pat[n] != 0;
    float v; int i;
    if (WAVE) {
        if (!real) { if (lane == 0) amax[n] = -1; return; }
        scan_row(y + (long)n * Lp, C, lane, 64, v, i);
        wave_best(v, i);
        if (lane == 0) amax[n] = i < C ? i : 0;
    } else {
        if (!real) { if (tid == 0) amax[n] = -1; return; }    // (workgroup-uniform)
        scan_row(y + (long)n * Lp, C, tid, 256, v, i);
        wave_best(v, i);
        if (lane == 0) { rv[wave] = v; ri[wave] = i; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w) take_better(v, i, rv[w], ri[w]);
            amax[n] = i < C ? i : 0;
        }
    }
}

__global__ __launch_bounds__(256) void ctc_collapse_kernel(CtcDecodeArgs a)
{
    extern __shared__ __align__(16) int diag[];               // three diagonals of a.maxShort + 1 ints
    __shared__ int red[4];
    const int slot = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int blank = a.C - 1;

    int cnt = 0;
    for (int t = tid; t < a.T; t += 256) cnt += a.pat[(long)t * a.PSp + slot] != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) red[wave] = cnt;
    __syncthreads();
    const int len = red[0] + red[1] + red[2] + red[3];
    __syncthreads();

    int *dec = a.decoded + (long)slot * a.T;
    int D = 0;                                                // (the same in every thread)
    for (int t0 = 0; t0 < len; t0 += 256) {
        const int t = t0 + tid;
        int k = -1;
        bool keep = false;
        if (t < len) {
            k = a.amax[(long)t * a.PSp + slot];
            const int before = t > 0 ? a.amax[(long)(t - 1) * a.PSp + slot] : -1;
            keep = k != blank && k != before;
        }
        const unsigned long long m = __ballot(keep);
        const int below = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) red[wave] = __popcll(m);
        __syncthreads();
        int base = D;
        for (int w = 0; w < wave; ++w) base += red[w];
        if (keep) dec[base + below] = k;                      // (base + below < len <= T)
        D += red[0] + red[1] + red[2] + red[3];
        __syncthreads();
    }
    if (tid == 0) a.decoded_len[slot] = D;
    if (!a.laboff) { if (tid == 0) a.dist[slot] = -1; return; }

    const int U = a.laboff[slot + 1] - a.laboff[slot];
    const int *lab = a.labels + a.laboff[slot];
    // x: the shorter sequence (index i, m of them), z: the longer one (index j, n of them); dec is this workgroup's own writes,
    // visible behind the barrier above
    const bool decShort = D <= U;
    const int *x = decShort ? dec : lab, *z = decShort ? lab : dec;
    const int m = decShort ? D : U, n = decShort ? U : D;
    const int w = a.maxShort + 1;
    int result = n;                                           // (m == 0: n insertions)
    if (m > 0) {
        for (int k = 0; k <= m + n; ++k) {
            int *cur = diag + (k % 3) * w;
            const int *p1 = diag + ((k + 2) % 3) * w, *p2 = diag + ((k + 1) % 3) * w;      // diagonals k - 1 and k - 2
            const int lo = k > n ? k - n : 0, hi = k < m ? k : m;
            for (int i = lo + tid; i <= hi; i += 256) {
                const int j = k - i;
                int v;
                if (i == 0 || j == 0) v = k;
                else {
                    const int sub = p2[i - 1] + (x[i - 1] != z[j - 1]);
                    const int gap = (p1[i - 1] < p1[i] ? p1[i - 1] : p1[i]) + 1;
                    v = sub < gap ? sub : gap;
                }
                cur[i] = v;
            }
            __syncthreads();
        }
        result = diag[((m + n) % 3) * w + m];
    }
    if (tid == 0) {
        a.dist[slot] = result;
        if (a.sums) {
            atomicAdd(a.sums, (unsigned long long)result);
            atomicAdd(a.sums + 1, (unsigned long long)U);
        }
    }
}

}  // namespace

bool ctc_decode_fits(int T, int max_labels)
{
    return std::min(T, max_labels) <= CTC_DECODE_MAX_SHORT;
}

void launch_ctc_argmax(hipStream_t s, const float *y, const char *pat, int N, int C, int Lp, int *amax)
{
    if (N <= 0) return;
    if (C <= CTC_ARGMAX_WAVE_C) hipLaunchKernelGGL(ctc_argmax_kernel<true>, dim3((N + 3) / 4), dim3(256), 0, s, y, pat, N, C, Lp, amax);
    else hipLaunchKernelGGL(ctc_argmax_kernel<false>, dim3(N), dim3(256), 0, s, y, pat, N, C, Lp, amax);
}

void launch_ctc_collapse(hipStream_t s, const CtcDecodeArgs &a)
{
    if (a.T <= 0 || a.PSp <= 0) return;
    const size_t lds = (size_t)3 * (a.maxShort + 1) * sizeof(int);
    hipLaunchKernelGGL(ctc_collapse_kernel, dim3(a.PSp), dim3(256), lds, s, a);
}

}  // namespace cn
