// Weight averaging (include/currennt_hip.h, section Weight averaging; no counterpart in the reference): an exponential moving
// average of the parameter arena's weights, and the exchange of the two around evaluation passes.  gfx950 only.
//
//   weight_average_kernel   avg[i] = copy ? w[i] : avg[i] + omd * (w[i] - avg[i]), three fp32 operations, each rounded on its own
//   weight_swap_kernel      w[i] <-> avg[i]
// Both are memory-bound streams over n floats (n a multiple of four, both pointers 16-byte aligned: every layer's offset and
// the arena's length are multiples of four floats): a lane owns 16 bytes, grid-stride loops, no LDS.
#include "cn_internal.h"

namespace cn {

// launch geometry: 256 lanes per workgroup, at most this many workgroups, 16 bytes per lane
constexpr int AVERAGE_THREADS = 256, AVERAGE_MAX_BLOCKS = 2048;
// elements one pass of a full grid covers; an arena longer than this takes the grid-stride loop's second round
constexpr size_t AVERAGE_PASS_ELEMS = (size_t)AVERAGE_MAX_BLOCKS * AVERAGE_THREADS * 4;

// (__fmul_rn / __fadd_rn are plain operators in this compiler's headers, and it fuses the product into the sum through them,
// pragma or not: the operators are written out here, under the pragma that keeps the three operations apart)
__device__ __forceinline__ float average_rule(float avg, float w, float omd)
{
#pragma clang fp contract(off)
    const float diff = w - avg;
    const float step = omd * diff;
    return avg + step;
}

template <bool COPY>
__global__ __launch_bounds__(AVERAGE_THREADS) void weight_average_kernel(float4 *__restrict__ avg, const float4 *__restrict__ w, size_t n4, float omd)
{
    const size_t nth = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += nth) {
        float4 x = w[i];
        if constexpr (!COPY) {
            const float4 a = avg[i];
            x.x = average_rule(a.x, x.x, omd); x.y = average_rule(a.y, x.y, omd);
            x.z = average_rule(a.z, x.z, omd); x.w = average_rule(a.w, x.w, omd);
        }
        avg[i] = x;
    }
}

__global__ __launch_bounds__(AVERAGE_THREADS) void weight_swap_kernel(float4 *__restrict__ w, float4 *__restrict__ avg, size_t n4)
{
    const size_t nth = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += nth) {
        const float4 a = avg[i], x = w[i];
        w[i] = a; avg[i] = x;
    }
}

static int average_blocks(size_t n4)
{
    if (n4 * 4 >= AVERAGE_PASS_ELEMS) return AVERAGE_MAX_BLOCKS;
    return (int)((n4 + AVERAGE_THREADS - 1) / AVERAGE_THREADS);
}

void launch_weight_average(hipStream_t s, float *avg, const float *w, size_t n, float omd, bool copy)
{
    const size_t n4 = n / 4;
    if (!n4) return;
    if (copy) hipLaunchKernelGGL(weight_average_kernel<true>, dim3(average_blocks(n4)), dim3(AVERAGE_THREADS), 0, s, (float4 *)avg, (const float4 *)w, n4, omd);
    else      hipLaunchKernelGGL(weight_average_kernel<false>, dim3(average_blocks(n4)), dim3(AVERAGE_THREADS), 0, s, (float4 *)avg, (const float4 *)w, n4, omd);
}

void launch_weight_swap(hipStream_t s, float *w, float *avg, size_t n)
{
    const size_t n4 = n / 4;
    if (!n4) return;
    hipLaunchKernelGGL(weight_swap_kernel, dim3(average_blocks(n4)), dim3(AVERAGE_THREADS), 0, s, (float4 *)w, (float4 *)avg, n4);
}

}  // namespace cn
