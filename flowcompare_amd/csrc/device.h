// Device-side idioms every kernel file shares, declared once: vector types, the LDS-DMA builtin, the lane swaps, the workgroup sum and compile-time loops.
// activations.h includes this header, so a kernel file that includes activations.h sees it already.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <utility>

namespace fc {

// ---------------------------------------------------------------- vector types (MFMA operands / accumulators, 16-byte moves)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- LDS-DMA (global_load_lds): global -> LDS without staging registers
// A wave instruction writes 64 consecutive units at the (wave-uniform) LDS address: lane l's unit lands at lds_dst + l * unit.
typedef __attribute__((address_space(3))) char lds_char;
typedef const __attribute__((address_space(1))) char glb_char;
__device__ __forceinline__ void lds_dma16(const void* global_src, void* lds_dst) {
    lds_char* dst = (lds_char*)lds_dst;      // (cast first: with both casts in the call premlp.hip's K = 160 kernels order two moves of a loop header differently)
    __builtin_amdgcn_global_load_lds((glb_char*)global_src, dst, 16, 0, 0);
}
__device__ __forceinline__ void lds_dma4(const float* global_src, float* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) float*)global_src, (__attribute__((address_space(3))) float*)lds_dst, 4, 0, 0);
}

// ---------------------------------------------------------------- lane swaps
// rows of 16 lanes (a0,a1,a2,a3 | b0,b1,b2,b3):  swap32 -> a = (a0,a1,b0,b1), b = (a2,a3,b2,b3) ;  swap16 -> a = (a0,b0,a2,b2), b = (a1,b1,a3,b3).
// Inline assembly: this hipcc's __builtin_amdgcn_permlane32_swap hands back its first result for both elements
// (profiles/micro/permlane32_swap_probe.hip); the s_nops cover the VALU <-> permlane-swap wait states the compiler cannot schedule around an
// asm block.  Two flavours, on purpose: swap32 / swap16 are `asm volatile` and keep their place among the memory operations around them;
// swap32_free is a plain `asm` the scheduler may move -- a volatile asm is a barrier for every memory operation in its dependence graph, which
// in mlprows.hip kept a stage's weight-fragment LDS reads (and with them its MFMAs) behind the swaps at the end of an epilogue quarter and
// serialised the quarter's VALU work and the stage's MFMAs (first build: 28 % matrix-pipe utilisation).
template <class T>
__device__ __forceinline__ void swap32(T& a, T& b) {
    static_assert(sizeof(T) == 4, "one 32-bit register per lane");
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}
template <class T>
__device__ __forceinline__ void swap16(T& a, T& b) {
    static_assert(sizeof(T) == 4, "one 32-bit register per lane");
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}
template <class T>
__device__ __forceinline__ void swap32_free(T& a, T& b) {
    static_assert(sizeof(T) == 4, "one 32-bit register per lane");
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}

// ---------------------------------------------------------------- per-scene key count of an attention launch (AttnProblem::m_counts, common.h)
// The keys scene b attends over: wave-uniform (blockIdx.y and kernel arguments only: a scalar load, pinned to an SGPR), and clamped into
// [1, M], because the host cannot check a device array without a synchronisation and a count must never become an out-of-range read.
__device__ __forceinline__ int attn_scene_keys(const int* m_counts, int b, int M) {
    if (!m_counts) return M;
    const int c = __builtin_amdgcn_readfirstlane(m_counts[b]);
    return c < 1 ? 1 : (c < M ? c : M);
}

// The points of scene b in a counted embedder launch (fcflow_embed_counts.h): the same scalar load, clamped into the bounds [lo, hi] the
// host vouches for and has chosen its kernels and grids by -- a device array that disagrees with them can reach neither a row past hi nor
// a kernel that was not launched.
__device__ __forceinline__ int scene_count(const int* m_counts, int b, int lo, int hi) {
    const int c = __builtin_amdgcn_readfirstlane(m_counts[b]);
    return c < lo ? lo : (c < hi ? c : hi);
}

// The rows scene b uses at one level of a counted PAConv launch (common.h: LevelCounts): its clamped count, divided by 4 once per level.
template <class LC>
__device__ __forceinline__ int level_count(const LC& c, int b) { return scene_count(c.counts, b, c.lo, c.hi) >> c.shift; }
// the same where b differs between the lanes of a wave (one thread per row): a vector load, no SGPR pin
template <class LC>
__device__ __forceinline__ int level_count_lane(const LC& c, int b) {
    const int v = c.counts[b];
    return (v < c.lo ? c.lo : (v < c.hi ? v : c.hi)) >> c.shift;
}

// ---------------------------------------------------------------- sum over a workgroup of up to 256 threads (the row kernels of training)
// deterministic: xor tree inside each wave, then waves in order.  red: blockDim.x / 64 floats of LDS; every thread gets the sum.
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) s += red[i];
    return s;
}

// ---------------------------------------------------------------- compile-time loop: f(integral_constant<int, 0>{}) ... f(integral_constant<int, N - 1>{})
template <class F, int... I>
__host__ __device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__host__ __device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

}  // namespace fc
