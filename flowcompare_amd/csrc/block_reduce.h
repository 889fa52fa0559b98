// Workgroup reductions of the staging kernels in a fixed order (bit-reproducible run to run), shared by staging.hip (co_unit_sphere_kernel,
// the change map) and scene_stage.hip (stage_pairs_counts_kernel) so that a pair normalised through either file gets the same bits:
// xor tree inside each wave, then the waves in ascending order.  red: blockDim.x / 64 floats of LDS; every thread gets the result.
#pragma once
#include <hip/hip_runtime.h>

namespace fc {

__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    return t;
}
__device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t = fmaxf(t, red[w]);
    return t;
}
__device__ __forceinline__ float block_min(float v, float* red) { return -block_max(-v, red); }

}  // namespace fc
