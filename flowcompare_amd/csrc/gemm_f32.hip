// The fp32-input MFMA main loop (VAR 2) and its kernels: the first build's loop, kept for A/B and tests; gemm.hip describes the variants.
#include "gemm_kernel.h"

namespace fc {

template <int BM, int BN, int WM, int WN, int TM, int TN>
__device__ __forceinline__ void mainloop_f32(const GemmParams& p, float* smem, floatx16 (&acc)[TM][TN], int tid, int wr, int wc, int li, int lh, int m0, int n0) {
    constexpr int NT = WM * WN * 64;
    constexpr int A_F4 = BM * 8 / NT, B_F4 = BN * 8 / NT, RPP = NT / 8;   // float4 per thread and tile; rows per staging pass
    constexpr int STAGE = gemm_stage_bytes<BM, BN, 2>() / (int)sizeof(float);   // floats: (BM + BN) rows of LDS_LD
    // ---- global -> register staging: thread t moves float4 (t&7) of rows (t>>3) + 32*i.  Straight-line code on plain register arrays (no
    //      conditionals around them: those sent the staging tile through scratch memory; the by-reference lambdas below do not -- same
    //      register figures, no scratch, in all six kernels).
    const int lrow = tid >> 3, lc4 = (tid & 7) * 4;
    float4 ra[A_F4], rb[B_F4];
    const float* wbase = p.W + (size_t)(n0 + lrow) * p.K_pad + lc4;
    const size_t wstep = (size_t)RPP * p.K_pad;
    float* const sAst = smem + lrow * LDS_LD + lc4;
    float* const sBst = sAst + BM * LDS_LD;

    auto gload = [&](int kt) {
        const float* Ap = p.A[0];
        int lda = p.lda[0], kk = kt;
        if (kk >= p.kt[0]) {
            kk -= p.kt[0]; Ap = p.A[1]; lda = p.lda[1];
            if (kk >= p.kt[1]) { kk -= p.kt[1]; Ap = p.A[2]; lda = p.lda[2]; }
        }
        const float* a = Ap + (size_t)(m0 + lrow) * lda + kk * 32 + lc4;
#pragma unroll
        for (int i = 0; i < A_F4; ++i) ra[i] = *reinterpret_cast<const float4*>(a + (size_t)(RPP * i) * lda);
        const float* w = wbase + kt * 32;
#pragma unroll
        for (int i = 0; i < B_F4; ++i) rb[i] = *reinterpret_cast<const float4*>(w + i * wstep);
    };
    auto lstore = [&](int stage) {
        float* sa = sAst + stage * STAGE;
        float* sb = sBst + stage * STAGE;
#pragma unroll
        for (int i = 0; i < A_F4; ++i) *reinterpret_cast<float4*>(sa + RPP * i * LDS_LD) = ra[i];
#pragma unroll
        for (int i = 0; i < B_F4; ++i) *reinterpret_cast<float4*>(sb + RPP * i * LDS_LD) = rb[i];
    };

    gload(0);
    lstore(0);
    __syncthreads();

    float4 af[2][TM], bf[2][TN];
    for (int kt = 0; kt < p.KT; ++kt) {
        const int ktn = kt + 1 < p.KT ? kt + 1 : kt;        // last iteration re-loads its own tile: keeps the loop branch free
        gload(ktn);
        const float* sA = smem + (kt & 1) * STAGE + (wr * TM * 32 + li) * LDS_LD + 4 * lh;
        const float* sB = smem + (kt & 1) * STAGE + BM * LDS_LD + (wc * TN * 32 + li) * LDS_LD + 4 * lh;
#pragma unroll
        for (int i = 0; i < TM; ++i) af[0][i] = *reinterpret_cast<const float4*>(sA + i * 32 * LDS_LD);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[0][j] = *reinterpret_cast<const float4*>(sB + j * 32 * LDS_LD);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int cb = g & 1, nb = cb ^ 1;
            if (g < 3) {                                   // fragments of the next 8-deep k group fly while this group's MFMAs run
#pragma unroll
                for (int i = 0; i < TM; ++i) af[nb][i] = *reinterpret_cast<const float4*>(sA + i * 32 * LDS_LD + 8 * (g + 1));
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[nb][j] = *reinterpret_cast<const float4*>(sB + j * 32 * LDS_LD + 8 * (g + 1));
            } else {
                lstore((kt + 1) & 1);                       // next tile's LDS image is written under the last group's MFMAs
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cb][i].x, bf[cb][j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cb][i].y, bf[cb][j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cb][i].z, bf[cb][j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cb][i].w, bf[cb][j].w, acc[i][j], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
}

template void launch_cfg<128, 64, 4, 1, EPI_LINEAR, 2>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 128, 2, 2, EPI_LINEAR, 2>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 320, 4, 1, EPI_LINEAR, 2>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 320, 4, 1, EPI_AFFINE, 2>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 320, 4, 1, EPI_AUGMENT, 2>(const GemmParams&, hipStream_t);
template void launch_cfg<128, 320, 4, 1, EPI_SLICE, 2>(const GemmParams&, hipStream_t);

}  // namespace fc
