// VAR 11: the fused spline layer as a persistent transposed LDS-DMA GEMM; gemm.hip describes the variants.
#include "gemm_kernel.h"

namespace fc {

// ===================================================================================================================================
// VAR 11: the fused spline layer as a PERSISTENT transposed LDS-DMA GEMM (K = 8 bins).  The tile is 128 x 128 on four waves stacked along
// the rows (32 points x 128 columns each) with the MFMA operands SWAPPED -- weights as the A operand, points as B -- so the accumulator
// holds, per lane, 64 parameters of ONE point (the other 64 sit in lane ^ 32).  With the column order of spline.h that is every parameter
// of 2-3 transformed dims in registers with compile-time indices: the spline is evaluated straight from the accumulators, the tile never
// goes through LDS (no 66 KB parameter tile, no transposition, no epilogue barrier).  Persistent because with one tile per workgroup the
// tile boundary is expensive: the in-kernel stamps (stamps, knob 20, profiles/micro/spline_gemm_stamps.py) priced it at 6.5 of a workgroup's 25.5 us
// per tile: 2.6 us from entry until the first k tile has landed, 0.8 us between a workgroup's exit and its successor's entry, 3.1 us of
// epilogue during which the slot fetches nothing.
//   * grid = 2 workgroups per CU, each walks tiles t = blockIdx.x, + gridDim.x, ... (the XCD-aware order of the one-tile-per-workgroup
//     launch: gridDim.x is a multiple of 8, so a workgroup's tiles stay on its XCD's band);
//   * ONE continuous DMA stream: behind the barrier of a tile's LAST k step the workgroup issues the NEXT tile's first k step into the
//     free stage (plus its 512 bytes of bias into LDS and its x2 / log-det operands into registers), so that data crosses the
//     epilogue in flight and the next tile's first barrier finds it landed;
//   * the epilogue never touches LDS and has no barrier: the four waves evaluate their splines independently, results stay in four
//     registers and are STORED behind the next tile's first barrier, so no wave waits for a store acknowledgement (stores count in
//     vmcnt on gfx9) before it may start multiplying again.
// LDS: 2 stages x 32 KB + 2 x 512 B of bias = 66560 B (two workgroups per CU).
__device__ __forceinline__ void spline_gemm_persistent(const GemmParams& p, float* smem) {
    constexpr int BM = 128, BN = 128, ROWB = gemm_row_bytes<11>(), STAGE = gemm_stage_bytes<BM, BN, 11>(), PPW = 8;
    static_assert(ROWB == 128 && 2 * (size_t)STAGE + 2 * 128 * sizeof(float) == gemm_lds_bytes<BM, BN, EPI_SPLINE, 11>(), "two stages and the two bias buffers, as launch_cfg reserves them");
    const GemmEpi& e = p.e;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* smc = reinterpret_cast<char*>(smem);
    float* biasbuf = smem + 2 * STAGE / 4;                              // [2][128]
    const int KT = p.KT;
    const unsigned rowbytes = (unsigned)KT * 128u;
    const int ntiles = p.nbm * p.nbn, G = gridDim.x;
    int t = blockIdx.x;
    if (t >= ntiles) return;

    // DMA pieces: piece pc = wave * 8 + i covers stage rows 8 pc .. 8 pc + 7 (rows 0..127: points, 128..255: weight rows); waves 0, 1 fetch
    // the points, waves 2, 3 the weights, so a wave's source base is scalar and its eight per-lane byte offsets never change
    unsigned poff[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int r = (wave * PPW + i) * 8 + (lane >> 3);
        const int cl = (lane & 7) ^ ((r >> 1) & 7);
        poff[i] = (unsigned)(r & (BM - 1)) * rowbytes + cl * 16;
    }
    auto src_of = [&](int bm, int bn) -> const char* {
        return wave < 2 ? reinterpret_cast<const char*>(e.A16) + (size_t)bm * BM * rowbytes : reinterpret_cast<const char*>(p.W2) + (size_t)bn * BN * rowbytes;
    };
#define FC_PDMA(SRC_, KT_, ST_)                                                                                       \
    {                                                                                                                 \
        const char* src_ = (SRC_) + (size_t)(KT_) * 128;                                                             \
        _Pragma("unroll") for (int i = 0; i < PPW; ++i)                                                              \
            lds_dma16(src_ + poff[i], smc + (ST_) * STAGE + (wave * PPW + i) * 1024);                             \
    }
    auto bias_dma = [&](int bn, int par) {                              // 128 floats: waves 0 and 1, 4 bytes per lane
        if (wave < 2)
            lds_dma4(p.bias + bn * BN + wave * 64 + lane, biasbuf + par * 128 + wave * 64);
    };
    auto load_x = [&](int bm, int bn, float (&x)[3], float& ldj) {
        const int row = bm * BM + wave * 32 + li, dim0 = bn * 5;
        const float* xr = e.xbuf + (size_t)row * e.ldx + e.x2_col0 + dim0;
        const bool rv = row < e.rows_valid;
        x[0] = rv && dim0 + 2 * lh < e.d2 ? xr[2 * lh] : 0.f;
        x[1] = rv && dim0 + 2 * lh + 1 < e.d2 ? xr[2 * lh + 1] : 0.f;
        x[2] = rv && dim0 + 4 < e.d2 ? xr[4] : 0.f;
        ldj = lh == 0 ? e.ldj_part[(size_t)bn * e.ldj_pitch + row] : 0.f;
    };
    int bm, bn;
    xcd_tile(p, t, bm, bn);
    const char* src = src_of(bm, bn);
    if (p.stamps && threadIdx.x == 0) {
        p.stamps[(size_t)t * 16 + 7] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
        p.stamps[(size_t)t * 16 + 8] = wall_clock64();
    }
    FC_STAMP_AT(t, 0)
    FC_PDMA(src, 0, 0)
    bias_dma(bn, 0);
    float spl_x[3], spl_ldj;
    load_x(bm, bn, spl_x, spl_ldj);
    FC_STAMP_AT(t, 1)

    floatx16 acc[4], corr[4];
    const int xsw = (li >> 1) & 7;
    const int a_row = (wave * 32 + li) * ROWB, b_row = (BM + li) * ROWB;
    int st = 0, par = 0;
    // results of the previous tile, stored behind this tile's first barrier
    bool pend = false;
    int pbm = 0, pbn = 0;
    float pyA = 0.f, pyB = 0.f, pyC = 0.f, pldj = 0.f;
    auto flush = [&]() {
        const int row = pbm * BM + wave * 32 + li, dim0 = pbn * 5;
        const bool rv = row < e.rows_valid;
        float* xr = e.xbuf + (size_t)row * e.ldx + e.x2_col0 + dim0;
        if (rv && dim0 + 2 * lh < e.d2) xr[2 * lh] = pyA;
        if (rv && dim0 + 2 * lh + 1 < e.d2) xr[2 * lh + 1] = pyB;
        if (rv && lh == 0 && dim0 + 4 < e.d2) xr[4] = pyC;
        if (lh == 0) e.ldj_part[(size_t)pbn * e.ldj_pitch + row] = pldj;
    };

    for (;;) {
        const int tn = t + G;
        const bool has_next = tn < ntiles;
        int nbm = 0, nbn = 0;
        if (has_next) xcd_tile(p, tn, nbm, nbn);
        float nx[3] = {0.f, 0.f, 0.f}, nldj = 0.f;
        for (int kt = 0; kt < KT; ++kt) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's pieces of this k step (and anything older) have landed
            __builtin_amdgcn_s_barrier();                               // ... everybody's have; everybody is done reading the other stage
            if (kt + 1 < KT) {                                          // the DMA runs one k step ahead
                // (readfirstlane keeps the step a scalar offset: with a plain kt + 1 hipcc carries the pieces' addresses as per-lane
                //  induction variables instead -- 256 VGPRs and 3 spilled, against 245 and none)
                FC_PDMA(src, __builtin_amdgcn_readfirstlane(kt + 1), (st ^ 1))
            } else if (has_next) {                                      // the stream runs on into the next tile
                src = src_of(nbm, nbn);
                FC_PDMA(src, 0, (st ^ 1))
                bias_dma(nbn, par ^ 1);
                load_x(nbm, nbn, nx, nldj);
            }
            if (kt == 0) {
                FC_STAMP_AT(t, 2)
                if (pend) flush();
                // accumulators start from the bias (transposed product: it varies along the accumulator's registers)
                const float* bb = biasbuf + par * 128 + 4 * lh;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 b4 = *reinterpret_cast<const float4*>(bb + j * 32 + 8 * g);
                        acc[j][4 * g + 0] = b4.x; acc[j][4 * g + 1] = b4.y; acc[j][4 * g + 2] = b4.z; acc[j][4 * g + 3] = b4.w;
                    }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) corr[j][r] = 0.f;
            }
            {
                const char* sA = smc + st * STAGE + a_row;
                const char* sB = smc + st * STAGE + b_row;
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    f16x8 xf[2], wf[4][2];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int off = ((sub * 4 + q * 2 + lh) ^ xsw) * 16;
                        xf[q] = *reinterpret_cast<const f16x8*>(sA + off);
#pragma unroll
                        for (int j = 0; j < 4; ++j) wf[j][q] = *reinterpret_cast<const f16x8*>(sB + j * 32 * ROWB + off);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j][0], xf[0], acc[j], 0, 0, 0);      // hi * hi
                        corr[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j][1], xf[0], corr[j], 0, 0, 0);    // lo' * hi
                        corr[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j][0], xf[1], corr[j], 0, 0, 0);    // hi * lo'
                    }
                }
            }
            st ^= 1;
        }
        FC_STAMP_AT(t, 3)
        // ---- epilogue in registers: slot s = 16 j + r of this lane is tile column spline_slot_col(s, lh): slots 0..24 / 25..49 are dims
        //      2 lh / 2 lh + 1, slots 50.. of the lower half are parameters 0..13 of dim 4, slots 50..60 of the upper half its parameters 14..24
        if (p.ablate != 2) {                                            // (diagnostic knob 14 = 2: main loop only)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] += corr[j][r] * (1.0f / 2048.0f);
            auto P = [&](int s) -> float { return acc[s >> 4][s & 15]; };
            float t4[11];
#pragma unroll
            for (int i = 0; i < 11; ++i) t4[i] = upper_to_lower(acc[3][2 + i]);      // slots 50..60 of the upper half: dim 4, parameters 14..24
            FC_STAMP_AT(t, 4)
            const int row = bm * BM + wave * 32 + li, dim0 = bn * 5;
            const bool rv = row < e.rows_valid;
            const bool vA = rv && dim0 + 2 * lh < e.d2, vB = rv && dim0 + 2 * lh + 1 < e.d2, vC = rv && lh == 0 && dim0 + 4 < e.d2;
            float lA, lB, lC;
            if (p.ablate == 1) {                                        // (diagnostic knob 14 = 1: no spline evaluation)
                pyA = spl_x[0] + P(0); lA = P(1); pyB = spl_x[1] + P(25); lB = P(26); pyC = spl_x[2] + P(50); lC = P(51);
            } else {
                rq_spline_fwd_regs<8>(spl_x[0], [&](int q) { return P(q); }, rq_unscaled{}, pyA, lA);
                rq_spline_fwd_regs<8>(spl_x[1], [&](int q) { return P(25 + q); }, rq_unscaled{}, pyB, lB);
                rq_spline_fwd_regs<8>(spl_x[2], [&](int q) { return q < 14 ? P(50 + q) : t4[q - 14]; }, rq_unscaled{}, pyC, lC);
            }
            lA = vA ? lA : 0.f; lB = vB ? lB : 0.f; lC = vC ? lC : 0.f;
            const float l2 = upper_to_lower(lA), l3 = upper_to_lower(lB);
            float sum = 0.f;
            sum += lA; sum += lB; sum += l2; sum += l3; sum += lC;      // dim order, like the LDS-tile epilogues (bit-identical slot values)
            pldj = spl_ldj + sum;
            pbm = bm; pbn = bn; pend = true;
            FC_STAMP_AT(t, 5)
        }
        if (p.stamps && threadIdx.x == 0) p.stamps[(size_t)t * 16 + 9] = wall_clock64();
        FC_STAMP_AT(t, 6)
        if (!has_next) break;
        t = tn; bm = nbm; bn = nbn; par ^= 1;
        spl_x[0] = nx[0]; spl_x[1] = nx[1]; spl_x[2] = nx[2]; spl_ldj = nldj;
        if (p.stamps && threadIdx.x == 0) {
            p.stamps[(size_t)t * 16 + 7] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
            p.stamps[(size_t)t * 16 + 8] = wall_clock64();
        }
        FC_STAMP_AT(t, 0)
        FC_STAMP_AT(t, 1)
    }
    if (pend) flush();
#undef FC_PDMA
}
template <>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void gemm_f32_kernel<128, 128, 4, 1, EPI_SPLINE, 11>(const GemmParams p) {
    extern __shared__ float smem[];
    spline_gemm_persistent(p, smem);
}
template void launch_cfg<128, 128, 4, 1, EPI_SPLINE, 11>(const GemmParams&, hipStream_t);

}  // namespace fc
