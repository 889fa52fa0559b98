// What every translation unit of the GEMM shares: parameters, tile order, LDS sizes, the kernel template (with the DMA and split main loops and
// the epilogues inline) and its launcher.  gemm.hip describes the variants; only the VAR 2 loop lives in the .hip file that instantiates it.
#pragma once
#include "common.h"
#include "activations.h"
#include "spline.h"
#include "launch.h"
#include <type_traits>
#include <cstdio>
#include <cstdlib>

namespace fc {

struct GemmParams {
    const float* A[3];
    int lda[3];
    int kt[3];          // 32-wide k tiles per segment
    int KT;             // total k tiles
    const float* W;     // [N_pad][K_pad]
    const unsigned short* W3;   // bf16 limb image [n_alloc][K_pad/16][3][16] (split-bf16 variant)
    const unsigned short* W2;   // fp16 limb image [n_alloc][K_pad/16][2][16]: hi, lo' = (w - hi) * 2048 (split-fp16 variant)
    int* ovf;                   // split-fp16 variant: set to 1 when an activation >= 65504 was met
    int K_pad;
    const float* bias;
    const float* colvec;
    int N_pad;
    int nbm, nbn;
    int col_group;      // > 0: row-band / column-group tile order for weight matrices that do not fit L2
    unsigned long long* stamps;   // diagnostic stamps (knob 20): 16 x u64 per workgroup (s_memtime at the phase boundaries, HW_ID, wall clock); null otherwise
    int ablate;         // diagnostic spline_ablate (knob 14), results invalid: 1 = no spline evaluation, 2 = main loop only, 3 = no parameter-tile write, 4 = no x2 store, 5 = stop behind the tile write; 0 otherwise
    GemmEpi e;
};


constexpr int LDS_LD = 36;   // floats per LDS row (32 + 4 pad)


// LDS of one launch, the one source the kernels' stage constants and launch_cfg share: stages x (BM + BN) rows of the loop's row pitch
// (VAR 11 adds two 512-byte bias buffers), or the fused spline epilogue's parameter tile where that is larger.
template <int VAR> constexpr int gemm_row_bytes() { return VAR == 9 || VAR == 11 ? 128 : VAR == 5 ? 80 : VAR == 3 ? 112 : LDS_LD * (int)sizeof(float); }
template <int BM, int VAR> constexpr int gemm_stages() { return VAR == 9 && BM == 64 ? 8 : 2; }
template <int BM, int BN, int VAR> constexpr int gemm_stage_bytes() { return (BM + BN) * gemm_row_bytes<VAR>(); }
template <int BM, int BN> constexpr size_t gemm_spline_tile_bytes() { return ((size_t)BM * (BN + 1) + (size_t)BM * 9) * sizeof(float); }   // tile + <= 9 dims of log-dets
template <int BM, int BN, int EPI, int VAR>
constexpr size_t gemm_lds_bytes() {
    const size_t lds_main = (size_t)gemm_stages<BM, VAR>() * gemm_stage_bytes<BM, BN, VAR>() + (VAR == 11 ? 1024 : 0);
    const size_t lds_epi = EPI == EPI_SPLINE && VAR != 11 ? gemm_spline_tile_bytes<BM, BN>() : 0;
    return lds_main > lds_epi ? lds_main : lds_epi;
}

// In-kernel phase stamps of the LDS-DMA kernels (diagnostic stamps, knob 20; profiles/micro/spline_gemm_stamps.py): thread 0 of a workgroup stores
// the shader-clock counter.  Slot 0 entry, 1 prologue issued, 2 first k tile landed, 3 main loop done, 4 epilogue operands ready (LDS tile
// written / register exchange done), 5 splines evaluated, 6 results stored, 7 HW_ID | XCC_ID << 32, 8 / 9 wall clock (100 MHz) at entry / exit.
#define FC_STAMP_AT(WG_, K_)                                                                                         \
    if (p.stamps && threadIdx.x == 0) {                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
        p.stamps[(size_t)(WG_) * 16 + (K_)] = __builtin_amdgcn_s_memtime();                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
    }
#define FC_STAMP(K_) FC_STAMP_AT(blockIdx.x, K_)

// Lanes 0..31 of the result receive lanes 32..63 of v (v_permlane32_swap_b32 swaps the upper half of its first operand with the lower
// half of its second; lanes 32..63 of the result are unspecified): device.h swap32.
__device__ __forceinline__ float upper_to_lower(float v) {
    float a = v, b = 0.f;
    swap32(a, b);
    return b;
}

// C/D layout of the 32x32 MFMA: column = lane & 31, row = mfma32_row(r, lane >> 5) for accumulator register r = 0..15
__device__ __forceinline__ constexpr int mfma32_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// XCD-aware tile order.  Blocks b, b+8, ... share an XCD (and its 4 MiB L2).
//  * small weight matrix (fits L2 beside the activations): each XCD takes a contiguous run of (row-tile, col-tile)
//    pairs with the col-tile fastest, so an A row panel is fetched from HBM once and W stays L2 resident;
//  * large weight matrix (p.col_group > 0, e.g. the 3750-wide spline parameter layer, W = 7.7 MB): each XCD owns a
//    band of row tiles and walks it in groups of col_group column tiles, so that group of W tiles stays in L2 while
//    the band's A panels stream past (measured before: 5x the algorithmic bytes were re-fetched through L2).
__device__ __forceinline__ void xcd_tile(const GemmParams& p, int b, int& bm, int& bn) {
    const int nb = p.nbm * p.nbn;
    const int xcd = b & 7, loc = b >> 3;
    if (p.col_group > 0) {
        const int rows_x = p.nbm >> 3, G = p.col_group;           // launcher guarantees nbm % 8 == 0
        const int g = loc / (rows_x * G);
        const int rem = loc - g * rows_x * G;
        const int w = p.nbn - g * G < G ? p.nbn - g * G : G;
        const int r = rem / w;
        bm = xcd * rows_x + r;
        bn = g * G + (rem - r * w);
    } else {
        const int q = nb >> 3, r = nb & 7;
        const int L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
        bm = L / p.nbn;
        bn = L - bm * p.nbn;
    }
}

// VAR 2, the fp32-input MFMA main loop: acc += A_tile @ W_tile^T over the k range.  Defined in gemm_f32.hip ONLY: every VAR 2 kernel must be
// instantiated there, behind the definition (other VARs discard the call under `if constexpr`).
template <int BM, int BN, int WM, int WN, int TM, int TN>
__device__ __forceinline__ void mainloop_f32(const GemmParams& p, float* smem, floatx16 (&acc)[TM][TN], int tid, int wr, int wc, int li, int lh, int m0, int n0);

// ---- LayerNorm folded through the layer (common.h): a wave's 64 columns are either hidden columns (sum of squares per row
//      into the block's slot) or the 64 q columns (stored un-normalised)
template <int TM, int TN>
__device__ __forceinline__ void epi_lnq(const GemmParams& p, const floatx16 (&acc)[TM][TN], int li, int lh, int wave_m0, int wave_n0) {
    const GemmEpi& e = p.e;
    static_assert(TN == 2, "LNQ epilogue: a wave owns one 64-column block (hidden columns or the q columns)");
    if (wave_n0 < e.d2) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float t = acc[i][0][r] * acc[i][0][r] + acc[i][1][r] * acc[i][1][r];
                t = half_wave_sum(t);
                if (li == 0) e.ldj_part[(size_t)(wave_n0 >> 6) * e.ldj_pitch + wave_m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh] = t;   // (spelled out: a size_t sum widens each term on its own; through mfma32_row the address code and the s_waitcnt count change)
            }
    } else if (wave_n0 < e.d2 + 64) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    e.C[(size_t)(wave_m0 + i * 32 + mfma32_row(r, lh)) * e.ldc + (wave_n0 - e.d2) + j * 32 + li] = acc[i][j][r];
    }
}

// The kernel reads: tile, prologue, main loop, epilogue.  Only the VAR 2 loop and the LNQ epilogue are functions; the other stages are
// inline blocks on purpose.  As __forceinline__ functions they compile to the same arithmetic in a different instruction order, and that
// changed s_waitcnt / ds counts or the spill count of some of the 26 instantiations (accumulator prologue, spline prefetch, DMA loop,
// split loop, LINEAR / SPLINE / pair epilogues: each was tried, alone and together).  Re-check per kernel before moving one out.
template <int BM, int BN, int WM, int WN, int EPI, int VAR = 2>
__global__ __launch_bounds__(WM * WN * 64) __attribute__((amdgpu_waves_per_eu(BN > 128 ? 1 : (BM == 128 && WM * WN == 8) ? 4 : 2)))   // resident waves per SIMD the register budget must allow
void gemm_f32_kernel(const GemmParams p) {
    constexpr int NT = WM * WN * 64;                       // 4 or 8 waves per workgroup
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    extern __shared__ float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave / WN, wc = wave % WN;
    const int li = lane & 31, lh = lane >> 5;

    // ---- tile
    int bm, bn;
    xcd_tile(p, blockIdx.x, bm, bn);
    const int m0 = bm * BM, n0 = bn * BN;
    const int wave_n0 = n0 + wc * TN * 32;
    const int wave_m0 = m0 + wr * TM * 32;
    int nvalid = (p.N_pad - wave_n0) / 32;                 // wave-uniform number of live 32-col tiles (for the stores only:
    nvalid = nvalid < 0 ? 0 : (nvalid > TN ? TN : nvalid); // W / bias are allocated zero-padded to the grid, the k-loop is branch free)
    const GemmEpi& e = p.e;
    if constexpr (VAR == 9) {
        if (p.stamps && threadIdx.x == 0) {
            p.stamps[(size_t)blockIdx.x * 16 + 7] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
            p.stamps[(size_t)blockIdx.x * 16 + 8] = wall_clock64();
        }
        FC_STAMP(0)
    }


    // ---- prologue
    // ---- accumulators start from the epilogue's additive terms (bias, rank-1 extra-context term, residual), so their
    //      global loads overlap the first tile's loads instead of forming a dependent tail after the last MFMA.
    //      Every runtime condition is hoisted OUTSIDE the unrolled element loops (a per-element "load or not" makes
    //      hipcc branch and wait vmcnt(0) around each load).
    // fused spline epilogue: the x2 values (and the log-det slot) this thread will update after the main loop are fetched NOW -- their
    // HBM latency then hides under the k loop instead of standing exposed between the tile's last MFMA and its spline evaluation
    constexpr int SPL_PER_THREAD = EPI == EPI_SPLINE ? (BM * 5 + NT - 1) / NT : 1;      // (K = 8: 5 dims per 128-column tile; K = 4 / 16 re-load below)
    float spl_x[SPL_PER_THREAD];
    float spl_ldj = 0.f;
    if constexpr (EPI == EPI_SPLINE) {
        const int per = 3 * e.spline_K + 1, DPT = BN / per, dim0 = bn * DPT;
#pragma unroll
        for (int k = 0; k < SPL_PER_THREAD; ++k) {
            const int it = tid + k * NT, row = it % BM, dl = it / BM;
            spl_x[k] = (DPT == 5 && it < BM * DPT && dim0 + dl < e.d2 && m0 + row < e.rows_valid)
                           ? e.xbuf[(size_t)(m0 + row) * e.ldx + e.x2_col0 + dim0 + dl] : 0.f;
        }
        if (tid < BM) spl_ldj = e.ldj_part[(size_t)bn * e.ldj_pitch + m0 + tid];
    }
    floatx16 acc[TM][TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        float bv = 0.f;
        if constexpr (EPI == EPI_LINEAR || EPI == EPI_SPLINE || EPI == EPI_LNQ) bv = p.bias ? p.bias[wave_n0 + j * 32 + li] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = bv;
    }
    if constexpr (EPI == EPI_LINEAR) {
        if (e.rowscal && p.colvec) {
            float rs[TM][16];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) rs[i][r] = e.rowscal[wave_m0 + i * 32 + mfma32_row(r, lh)];
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float cv = p.colvec[wave_n0 + j * 32 + li];
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] += rs[i][r] * cv;
            }
        }
        // (a residual that arrives as a limb image, e.residual16, is added BEHIND the k loop -- in the epilogue below: the row-resident chain
        // kernel (mlprows.hip) adds it there, and the engine picks between that kernel and these per-layer launches by the row count, so the
        // two must round alike for a scene's log-probs not to depend on the batch it sits in; it is also the more accurate order)
        if (e.residual) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (j < nvalid) {
                    const float* rp = e.residual + (size_t)(wave_m0 + 4 * lh) * e.ldr + wave_n0 + j * 32 + li;
                    float t[TM][16];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) t[i][r] = rp[(size_t)(i * 32 + mfma32_row(r, 0)) * e.ldr];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[i][j][r] += t[i][r];
                }
            }
        }
    }

    // 64 x 64 tiles (one 32 x 32 block per wave): the limb-image residual is requested HERE, in front of the k loop, and added behind it as in
    // every other tile shape -- such a launch lasts one workgroup's life (~9 us), and 32 two-byte loads issued in the epilogue were ~0.7 us of it
    constexpr bool RES_EARLY = EPI == EPI_LINEAR && VAR == 9 && TM == 1 && TN == 1;
    unsigned short res_h[RES_EARLY ? 16 : 1], res_l[RES_EARLY ? 16 : 1];
    if constexpr (RES_EARLY) {
        if (e.residual16 && nvalid > 0) {
            const int blocks = e.ldr16 >> 4;
            const int col = wave_n0 + li;
            const unsigned short* rp = e.residual16 + ((size_t)(wave_m0 + 4 * lh) * blocks + (col >> 4)) * 32 + (col & 15);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned short* q = rp + (size_t)(mfma32_row(r, 0)) * blocks * 32;
                res_h[r] = q[0]; res_l[r] = q[16];
            }
        }
    }

    // ---- main loop
    if constexpr (VAR == 9) {
        // ================= split-fp16 main loop on LDS-DMA: BOTH operands arrive as fp16 limb images =================
        // A is the image its producer's epilogue wrote (e.A16, [rows][K/16][hi 16 | lo' 16]), W the host-packed one (p.W2): the main
        // loop converts nothing, so global -> LDS is a byte copy and goes through `global_load_lds_dwordx4` (no staging VGPRs, no
        // ds_write, whose VGPR -> LDS path was half busy in the register-staged loop).  128 x 128 tile on FOUR waves of 64 x 64 (128
        // accumulator registers: main + cross-product sets); k tile 32 = two 64-byte (row, k16) blocks = 128 bytes per LDS row; TWO LDS
        // stages of 32 KB, so that two workgroups fit a CU (2 x 64 KB of stages / 2 x 69 KB with the spline epilogue's parameter tile;
        // 2 waves per SIMD): one workgroup's epilogue then overlaps the other's main loop; ONE raw s_barrier per k tile.
        //   LDS image: row r = 128 bytes = 8 chunks of 16 B; logical chunk c = 4*(k16 block) + 2*limb + (k half) sits at physical
        //   chunk c ^ ((r >> 1) & 7): with 128-byte rows two rows share a 256-byte bank row, and ds_read_b128's 16-lane groups
        //   ({0-3,12-15,20-27}, ...) then hit 16 distinct 16-byte slots.  The DMA writes LDS linearly (wave base + lane * 16), so the
        //   permutation is applied to the per-lane SOURCE address and again on the read (same involution on both sides).
        static_assert((BN == 128 && BM == 128 && WM == 2 && WN == 2) ||
                          (BM == 64 && BN == 64 && WM == 2 && ((WN == 2 && EPI == EPI_LINEAR) || (WN == 1 && EPI == EPI_AFFINE))),
                      "LDS-DMA loop: 128x128 on 2x2 waves; 64x64 on 2x2 waves (EPI_LINEAR) / 2x1 waves (EPI_AFFINE: a wave's 64 columns are one "
                      "pair block) for launches too small to fill the chip with 128x128 tiles");
        // 64 x 64 tiles (launches too small to fill the chip: ONE workgroup's k loop is the launch's duration, and with 6 MFMAs per wave and
        // k step that loop is pure DMA latency): EIGHT stages of 16 KB, seven k steps in flight, so the whole K = 512 operand is on its way
        // after one latency instead of one latency per k step (C1: 19 -> ~10 us per hidden-layer launch).  Same MFMAs in the same order.
        constexpr int NST8 = gemm_stages<BM, VAR>();
        constexpr int ROWB8 = gemm_row_bytes<VAR>(), STAGE8 = gemm_stage_bytes<BM, BN, VAR>();
        static_assert(ROWB8 == 128 && (size_t)NST8 * STAGE8 <= gemm_lds_bytes<BM, BN, EPI, VAR>(), "the swizzle below is built for 128-byte rows; launch_cfg reserves the stages");
        constexpr int PPW = STAGE8 / 1024 / (NT / 64);                       // 1-KB DMA pieces per wave and stage: 8 on the 128 x 128 tile
        char* smc = reinterpret_cast<char*>(smem);
        const int KT = p.KT;                                                // k32 tiles
        const size_t rowbytes = (size_t)KT * 128;
        // piece pc = wave * PPW + i covers stage rows 8 pc .. 8 pc + 7 (rows 0..BM-1: A, then W); lane l: row 8 pc + (l >> 3), physical chunk l & 7
        const char* gsrc[PPW];
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int pc = wave * PPW + i;
            const int r = pc * 8 + (lane >> 3);
            const int cl = (lane & 7) ^ ((r >> 1) & 7);
            const char* base = pc < BM / 8 ? reinterpret_cast<const char*>(e.A16) + (size_t)(m0 + r) * rowbytes
                                           : reinterpret_cast<const char*>(p.W2) + (size_t)(n0 + r - BM) * rowbytes;
            gsrc[i] = base + cl * 16;
        }
#define FC_DMA8(KT_, ST_)                                                                                          \
        {                                                                                                          \
            _Pragma("unroll") for (int i = 0; i < PPW; ++i)                                                        \
                lds_dma16(gsrc[i] + (size_t)(KT_) * 128, smc + (ST_) * STAGE8 + (wave * PPW + i) * 1024);          \
        }
        floatx16 corr[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) corr[i][j][r] = 0.f;
        const int xsw = (li >> 1) & 7;                                      // (row >> 1) & 7 of every row this lane reads (tiles are 32-row aligned)
        const int a_row = (wr * TM * 32 + li) * ROWB8, b_row = (BM + wc * TN * 32 + li) * ROWB8;
#define FC_MMA8_STAGE(ST_)                                                                                         \
        {                                                                                                          \
            const char* sA = smc + (ST_) * STAGE8 + a_row;                                                         \
            const char* sB = smc + (ST_) * STAGE8 + b_row;                                                         \
            _Pragma("unroll") for (int sub = 0; sub < 2; ++sub) {                                                  \
                f16x8 af8[TM][2], bf8[TN][2];                                                                      \
                _Pragma("unroll") for (int q = 0; q < 2; ++q) {                                                    \
                    const int off = ((sub * 4 + q * 2 + lh) ^ xsw) * 16;                                           \
                    _Pragma("unroll") for (int i = 0; i < TM; ++i) af8[i][q] = *reinterpret_cast<const f16x8*>(sA + i * 32 * ROWB8 + off); \
                    _Pragma("unroll") for (int j = 0; j < TN; ++j) bf8[j][q] = *reinterpret_cast<const f16x8*>(sB + j * 32 * ROWB8 + off); \
                }                                                                                                  \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                     \
                    _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                               \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af8[i][0], bf8[j][0], acc[i][j], 0, 0, 0);     /* hi * hi */  \
                        corr[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af8[i][0], bf8[j][1], corr[i][j], 0, 0, 0);   /* hi * lo' */ \
                        corr[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af8[i][1], bf8[j][0], corr[i][j], 0, 0, 0);   /* lo' * hi */ \
                    }                                                                                              \
            }                                                                                                      \
        }
        if constexpr (NST8 > 3) {
            constexpr int DEPTH = NST8 - 1;
            static_assert((DEPTH - 1) * PPW <= 63, "counted vmcnt wait");
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) FC_DMA8((d < KT ? d : KT - 1), d)
            int st = 0;
            for (int kt = 0; kt < KT; ++kt) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DEPTH - 1) * PPW) : "memory");   // this wave's pieces of tile kt have landed (DEPTH - 1 younger tiles may fly on)
                __builtin_amdgcn_s_barrier();                                   // ... and everybody's; everybody is done reading tile kt-1
                const int kn = kt + DEPTH < KT ? kt + DEPTH : KT - 1;           // (tail: harmless re-loads into the stage tile kt-1 just left)
                const int sn = st == 0 ? NST8 - 1 : st - 1;                     // (kt + DEPTH) % NST8
                FC_DMA8(kn, sn)
                FC_MMA8_STAGE(st)
                st = st == NST8 - 1 ? 0 : st + 1;
            }
        } else {
            // two stages: tile kt+1 is in flight while tile kt is multiplied (issued right behind the barrier that frees its stage)
            FC_DMA8(0, 0)
            FC_STAMP(1)
            int st = 0;
            for (int kt = 0; kt < KT; ++kt) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (kt == 0) FC_STAMP(2)
                if (kt + 1 < KT) FC_DMA8(kt + 1, (st ^ 1))
                FC_MMA8_STAGE(st)
                st ^= 1;
            }
        }
#undef FC_MMA8_STAGE
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // the tail's re-loads: nothing may land in LDS once the epilogue owns it
        __syncthreads();
        FC_STAMP(3)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += corr[i][j][r] * (1.0f / 2048.0f);
#undef FC_DMA8
    } else if constexpr (VAR >= 3) {
        // ================= split-bf16 main loop: fp32-equivalent products on the bf16 matrix cores =================
        // x = hi + mid + lo (three bf16 limbs, 24 significant bits);  a*b ~= ah*bh + (ah*bm + am*bh) + (ah*bl + am*bm + al*bh),
        // the dropped terms are below 2^-24 |a b|.  Every limb product is exact in the MFMA's fp32 accumulator, so the result
        // has fp32-GEMM accuracy (profiles/micro: 6e-9 rel. error with exact accumulation) at 6 bf16 MFMAs (32 cycles each)
        // per 32x32x16 block instead of 8 fp32 MFMAs (64 cycles each): 2.67x the matrix rate.  Weights are pre-split on the host
        // (PackedLinear.W3); activations are split while they are staged into LDS.  K tile = 16, LDS row = 3 limbs x 32 B + 16 B pad.
        //
        // VAR 5, the default: TWO fp16 limbs.  x = hi + lo'/2048 with hi = rn16(x), lo' = rn16((x - hi) * 2048): hi carries 11 bits,
        // the scaled remainder the next 11 (+ sign), so the pair represents x to 2^-24 relative -- fp32's own rounding unit -- and
        // the scaling keeps lo' out of fp16's subnormal range (abs. error floor 2^-36 per element).  a*b ~= ah*bh + (ah*bl' +
        // al'*bh)/2048: the h*h products go to the main accumulator, the two cross products to a second one that is scaled by
        // 2^-11 (exact) and added once after the k loop; the dropped l*l term is < 2^-24 |a b|.  3 MFMAs per block instead of 6
        // (5.3x the fp32-input matrix rate), 4 bytes per LDS element instead of 6.  fp16 overflows at 65504: every staged |x| is
        // max-reduced and a launch that met one >= 65504 raises *p.ovf; the entry point then repeats the whole call with the
        // bf16 limbs (unbounded range).  Weights with such entries never get an fp16 image (PackedLinear.W2 == nullptr).
        constexpr bool F16 = VAR == 5;
        constexpr int KS = 16;                                      // k extent of one LDS stage (32 with one-deep prefetch measured 13 % slower)
        constexpr int KSUB = KS / 16, U = 32 / KS;
        constexpr int NL = F16 ? 2 : 3;                             // limbs
        constexpr int LIMB_B = KS * 2;                              // bytes of one limb of a row
        constexpr int ROWB = NL * LIMB_B + 16;                      // bytes per LDS row (16 B pad: conflict-free 16-byte fragment reads)
        constexpr int CH = NL * KS / 8;                             // 16-byte chunks per (row, stage) of a limb image
        constexpr int STAGE3 = gemm_stage_bytes<BM, BN, VAR>();
        static_assert(ROWB == gemm_row_bytes<VAR>() && 2 * (size_t)STAGE3 <= gemm_lds_bytes<BM, BN, EPI, VAR>(), "row pitch of gemm_row_bytes; launch_cfg reserves two stages");
        constexpr int TPR = KS / 4;                                 // threads (float4s) per A row
        constexpr int RPP3 = NT / TPR, A3 = BM / RPP3, W3N = (BN * CH + NT - 1) / NT;   // float4 loads of A, 16-byte loads of W per thread and stage
        char* smc = reinterpret_cast<char*>(smem);
        // Row slots are dealt to lanes so that the lanes one LDS store cycle serves (16 for ds_write_b64, 8 for ds_write_b128;
        // stores see 32 banks) fall on distinct banks of the 80-byte-pitch image: with the natural order rows r and r+3 (b64)
        // or r and r+1 (b128) overlapped, a 2-way conflict on the CU's scarcest path (VGPR -> LDS, ~80 B/clk).
        const int rs3 = tid / TPR;
        const int lrow3 = F16 ? 8 * (rs3 >> 3) + ((rs3 >> 2) & 1) + 2 * (rs3 & 3) : rs3, lc3 = (tid % TPR) * 4;
#define FC_WROW(SLOT_) (F16 ? 8 * ((SLOT_) >> 3) + (((SLOT_) >> 1) & 3) + 4 * ((SLOT_) & 1) : (SLOT_))
        const int KT16 = p.KT * 2;
        const unsigned short* const Wl = F16 ? p.W2 : p.W3;
        float amax = 0.f;
        // two register sets: the tile loaded in iteration kt is only converted/stored in iteration kt+1, so a global load has a
        // whole iteration (the MFMAs of the other resident waves included) to land before anything waits for it
        float4 ra3_0[A3], ra3_1[A3];
        typedef unsigned int u32xw __attribute__((ext_vector_type(4 * W3N)));      // whole-vector values: never an alloca, so never scratch
        u32xw rw3_0, rw3_1;
#define FC_GLOAD3(S_, KT_)                                                                                           \
        {                                                                                                          \
            const float* Ap_ = p.A[0];                                                                             \
            int lda_ = p.lda[0], kk_ = (KT_);                                                                      \
            if (kk_ >= U * p.kt[0]) {                                                                              \
                kk_ -= U * p.kt[0]; Ap_ = p.A[1]; lda_ = p.lda[1];                                                 \
                if (kk_ >= U * p.kt[1]) { kk_ -= U * p.kt[1]; Ap_ = p.A[2]; lda_ = p.lda[2]; }                     \
            }                                                                                                      \
            const float* a_ = Ap_ + (size_t)(m0 + lrow3) * lda_ + kk_ * KS + lc3;                                  \
            _Pragma("unroll") for (int i = 0; i < A3; ++i) ra3_##S_[i] = *reinterpret_cast<const float4*>(a_ + (size_t)(RPP3 * i) * lda_); \
            _Pragma("unroll") for (int i = 0; i < W3N; ++i) {                                                      \
                int c_ = tid + NT * i;                                                                             \
                c_ = c_ < BN * CH ? c_ : BN * CH - 1;     /* unconditional load (a guarded one sends the staging registers through scratch) */ \
                const int slot_ = c_ / CH, part_ = c_ - slot_ * CH, row_ = FC_WROW(slot_);                         \
                const int sub_ = part_ / (NL * 2), q2_ = part_ - sub_ * (NL * 2);   /* k16 tile of the stage; limb*2 + half */ \
                const uint4 t_ = *reinterpret_cast<const uint4*>(Wl + ((size_t)(n0 + row_) * KT16 + (KT_) * KSUB + sub_) * (NL * 16) + q2_ * 8); \
                rw3_##S_[4 * i] = t_.x; rw3_##S_[4 * i + 1] = t_.y; rw3_##S_[4 * i + 2] = t_.z; rw3_##S_[4 * i + 3] = t_.w; \
            }                                                                                                      \
        }
#define FC_LSTORE3(S_, ST_)                                                                                          \
        {                                                                                                          \
            char* sa_ = smc + (ST_) * STAGE3 + lrow3 * ROWB + (tid % TPR) * 8;                                      \
            _Pragma("unroll") for (int i = 0; i < A3; ++i) {                                                       \
                const float x_[4] = {ra3_##S_[i].x, ra3_##S_[i].y, ra3_##S_[i].z, ra3_##S_[i].w};                  \
                if constexpr (F16) {                                                                               \
                    amax = fmaxf(fmaxf(amax, fmaxf(fabsf(x_[0]), fabsf(x_[1]))), fmaxf(fabsf(x_[2]), fabsf(x_[3])));  \
                    uint2 h_, l_;                                  /* five VALU per pair of values (activations.h limb_split2) */ \
                    limb_split2(x_[0], x_[1], h_.x, l_.x);                                                         \
                    limb_split2(x_[2], x_[3], h_.y, l_.y);                                                         \
                    *reinterpret_cast<uint2*>(sa_ + RPP3 * i * ROWB) = h_;                                          \
                    *reinterpret_cast<uint2*>(sa_ + RPP3 * i * ROWB + LIMB_B) = l_;                                 \
                } else {                                                                                           \
                    bf16x4 h_, m_, l_;                                                                             \
                    _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) {                                             \
                        h_[e_] = (__bf16)x_[e_];                                                                   \
                        const float r1_ = x_[e_] - (float)h_[e_];                                                  \
                        m_[e_] = (__bf16)r1_;                                                                      \
                        l_[e_] = (__bf16)(r1_ - (float)m_[e_]);                                                    \
                    }                                                                                              \
                    *reinterpret_cast<bf16x4*>(sa_ + RPP3 * i * ROWB) = h_;                                         \
                    *reinterpret_cast<bf16x4*>(sa_ + RPP3 * i * ROWB + LIMB_B) = m_;                                \
                    *reinterpret_cast<bf16x4*>(sa_ + RPP3 * i * ROWB + 2 * LIMB_B) = l_;                            \
                }                                                                                                  \
            }                                                                                                      \
            _Pragma("unroll") for (int i = 0; i < W3N; ++i) {                                                      \
                const int c_ = tid + NT * i, slot_ = c_ / CH, part_ = c_ - slot_ * CH, row_ = FC_WROW(slot_);      \
                const int sub_ = part_ / (NL * 2), q2_ = part_ - sub_ * (NL * 2);                                  \
                if (BN * CH % NT == 0 || c_ < BN * CH)                                                             \
                    *reinterpret_cast<uint4*>(smc + (ST_) * STAGE3 + (BM + row_) * ROWB + (q2_ >> 1) * LIMB_B + sub_ * 32 + (q2_ & 1) * 16) = \
                        make_uint4(rw3_##S_[4 * i], rw3_##S_[4 * i + 1], rw3_##S_[4 * i + 2], rw3_##S_[4 * i + 3]);   \
            }                                                                                                      \
        }
#define FC_MMA3(ST_)                                                                                              \
        _Pragma("unroll") for (int sub = 0; sub < KSUB; ++sub) {                                                   \
            const char* sA = smc + (ST_) * STAGE3 + (wr * TM * 32 + li) * ROWB + lh * 16 + sub * 32;                \
            const char* sB = smc + (ST_) * STAGE3 + (BM + wc * TN * 32 + li) * ROWB + lh * 16 + sub * 32;           \
            if constexpr (F16) {                                                                                   \
                f16x8 af3[TM][2], bf3[TN][2];                                                                      \
                _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                     \
                    _Pragma("unroll") for (int q = 0; q < 2; ++q) af3[i][q] = *reinterpret_cast<const f16x8*>(sA + i * 32 * ROWB + q * LIMB_B); \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                     \
                    _Pragma("unroll") for (int q = 0; q < 2; ++q) bf3[j][q] = *reinterpret_cast<const f16x8*>(sB + j * 32 * ROWB + q * LIMB_B); \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                     \
                    _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                               \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af3[i][0], bf3[j][0], acc[i][j], 0, 0, 0);     /* hi * hi */  \
                        corr[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af3[i][0], bf3[j][1], corr[i][j], 0, 0, 0);   /* hi * lo' */ \
                        corr[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af3[i][1], bf3[j][0], corr[i][j], 0, 0, 0);   /* lo' * hi */ \
                    }                                                                                              \
            } else {                                                                                               \
                bf16x8 af3[TM][3], bf3[TN][3];                                                                     \
                _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                     \
                    _Pragma("unroll") for (int q = 0; q < 3; ++q) af3[i][q] = *reinterpret_cast<const bf16x8*>(sA + i * 32 * ROWB + q * LIMB_B); \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                     \
                    _Pragma("unroll") for (int q = 0; q < 3; ++q) bf3[j][q] = *reinterpret_cast<const bf16x8*>(sB + j * 32 * ROWB + q * LIMB_B); \
                _Pragma("unroll") for (int j = 0; j < TN; ++j)                                                     \
                    _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                               \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af3[i][2], bf3[j][0], acc[i][j], 0, 0, 0);   /* lo * hi */   \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af3[i][1], bf3[j][1], acc[i][j], 0, 0, 0);   /* mid * mid */ \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af3[i][0], bf3[j][2], acc[i][j], 0, 0, 0);   /* hi * lo */   \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af3[i][1], bf3[j][0], acc[i][j], 0, 0, 0);   /* mid * hi */  \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af3[i][0], bf3[j][1], acc[i][j], 0, 0, 0);   /* hi * mid */  \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af3[i][0], bf3[j][0], acc[i][j], 0, 0, 0);   /* hi * hi */   \
                    }                                                                                              \
            }                                                                                                      \
        }
        floatx16 corr[F16 ? TM : 1][F16 ? TN : 1];
        if constexpr (F16) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) corr[i][j][r] = 0.f;
        }
        // KT16 is even (K_pad is a multiple of 32).  Stage s of LDS holds tile kt (s = kt & 1); register set s holds tile kt+1 ... kt+2.
        FC_GLOAD3(0, 0)
        FC_LSTORE3(0, 0)
        FC_GLOAD3(1, 1)
        __syncthreads();
        for (int kt = 0; kt < KT16; kt += 2) {
            const int k2 = kt + 2 < KT16 ? kt + 2 : KT16 - 1, k3 = kt + 3 < KT16 ? kt + 3 : KT16 - 1;   // tail re-loads: branch-free loop
            FC_GLOAD3(0, k2)
            FC_MMA3(0)
            FC_LSTORE3(1, 1)
            __syncthreads();
            FC_GLOAD3(1, k3)
            FC_MMA3(1)
            FC_LSTORE3(0, 0)
            __syncthreads();
        }
        if constexpr (F16) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] += corr[i][j][r] * (1.0f / 2048.0f);
            if (amax >= 65504.0f) atomicOr(p.ovf, 1);               // some |x| does not fit fp16: the caller repeats with bf16 limbs
        }
#undef FC_MMA3
#undef FC_WROW
#undef FC_GLOAD3
#undef FC_LSTORE3
    } else mainloop_f32<BM, BN, WM, WN>(p, smem, acc, tid, wr, wc, li, lh, m0, n0);

    // ------------------------------------------------------------------ epilogues
    // C/D layout of the 32x32 MFMA: column = lane & 31, row = mfma32_row(r, lane >> 5), r = 0..15
    if constexpr (EPI == EPI_LINEAR) {
        if (VAR == 9 && p.ablate == 2) return;         // (diagnostic spline_ablate, knob 14, = 2: main loop only, results invalid)
        if constexpr (RES_EARLY) {
            if (e.residual16 && nvalid > 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    acc[0][0][r] += (float)__builtin_bit_cast(_Float16, res_h[r]) + (float)__builtin_bit_cast(_Float16, res_l[r]) * (1.0f / 2048.0f);
            }
        } else if (e.residual16) {
            // residual from the limb image its producer wrote (hidden activations of a limb-chained MLP exist only in that form): v = (bias + sum) + residual
            const int blocks = e.ldr16 >> 4;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (j < nvalid) {
                    const int col = wave_n0 + j * 32 + li;
                    const unsigned short* rp = e.residual16 + ((size_t)(wave_m0 + 4 * lh) * blocks + (col >> 4)) * 32 + (col & 15);
                    unsigned short th[TM][16], tl[TM][16];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const unsigned short* q = rp + (size_t)(i * 32 + mfma32_row(r, 0)) * blocks * 32;
                            th[i][r] = q[0]; tl[i][r] = q[16];
                        }
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            acc[i][j][r] += (float)__builtin_bit_cast(_Float16, th[i][r]) + (float)__builtin_bit_cast(_Float16, tl[i][r]) * (1.0f / 2048.0f);
                }
            }
        }

        // The activation and the output format are wave-uniform run-time values: they are dispatched ONCE, outside the element loops
        // (a `switch (act)` per element compiled to ~12 branches per output value -- incl. the ELU path's expm1f -- and cost the
        // 256x128 tile 18 us per tile, 40 % of a 512 -> 512 layer; round 2).  Each body below is straight-line code over the tile.
        float omax = 0.f;
        // 64-bit bases once per wave, 32-bit offsets inside the tile (a size_t product per element cost two 64-bit multiply-adds each)
        float* const cbase = e.C ? e.C + (size_t)wave_m0 * e.ldc + wave_n0 : nullptr;
        // the training epilogues (pre-activation copy, activation gradient) exist on the fp32-A loops only -- the ones the fc_train_* entries launch
        constexpr bool TRAIN_EPI = VAR == 2 || VAR == 3 || VAR == 5;
        float* const pbase = e.Cpre ? e.Cpre + (size_t)wave_m0 * e.ldc + wave_n0 : nullptr;
        const float* const gbase = e.gradu ? e.gradu + (size_t)wave_m0 * e.ldgu + wave_n0 : nullptr;
        const int rp16 = (p.N_pad >> 4) * 32;                          // ushorts per row of the limb image
        unsigned short* const hbase = e.C16 ? e.C16 + (size_t)wave_m0 * rp16 + (size_t)(wave_n0 >> 4) * 32 : nullptr;
        const float c16_s1 = e.c16_scale > 0.f ? e.c16_scale : 1.0f, c16_s2 = e.c16_scale > 0.f ? 1.0f : 2048.0f;
        auto body = [&](auto act_tag, auto fmt_tag) {
            constexpr int ACT = decltype(act_tag)::value;             // 16 + a: no activation, the value is multiplied by act_a'(gradu[row][col]) instead
            constexpr int FMT = decltype(fmt_tag)::value;             // 1: fp32 C, 2: limb image C16, 3: both; 5: fp32 C + the pre-activation value in Cpre
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (j < nvalid) {
                    const int cl = j * 32 + li;                       // column inside the wave's strip
                    const int c0 = cl & ~1;
                    const int hoff = (c0 >> 4) * 32 + ((li & 1) ? 16 : 0) + (c0 & 15);
                    float gu[ACT >= 16 ? TM : 1][16];                 // the block's act' arguments, requested up front (independent loads)
                    if constexpr (ACT >= 16) {
#pragma unroll
                        for (int i = 0; i < TM; ++i)
#pragma unroll
                            for (int r = 0; r < 16; ++r) gu[i][r] = gbase[(i * 32 + mfma32_row(r, lh)) * e.ldgu + cl];
                    }
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int rl = i * 32 + mfma32_row(r, lh);      // row inside the wave's strip
                            float v = acc[i][j][r];
                            if constexpr (ACT >= 16) v *= fc_act_grad(gu[i][r], ACT - 16);
                            if constexpr ((FMT & 4) != 0) pbase[rl * e.ldc + cl] = v;
                            v = fc_act<ACT>(v);                  // (the 16 + gact codes of the line above: identity)
                            if constexpr (FMT & 1) cbase[rl * e.ldc + cl] = v;
                            if constexpr (FMT & 2) {
                                // the output ALSO / ONLY as the fp16 limb image a following split-fp16 GEMM copies (its 30 column tiles
                                // would each re-split the same rows): lanes (c, c+1) swap one half through a DPP quad permute
                                // ([1,0,3,2]: a VALU move, not the LDS round trip __shfl_xor compiles to) and store one 32-bit word each
                                // (c16_s1, c16_s2) = (1, 2048): x = hi + lo'/2048; (kOneAccActScale, 1): the one-accumulator form hi + lo of x s1 (common.h)
                                const float vs = v * c16_s1;
                                omax = fmaxf(omax, fabsf(vs));
                                const _Float16 hb = (_Float16)vs;
                                const _Float16 lb = (_Float16)((vs - (float)hb) * c16_s2);
                                const unsigned hu = __builtin_bit_cast(unsigned short, hb), lu = __builtin_bit_cast(unsigned short, lb);
                                const unsigned mine = (li & 1) ? lu : hu, give = (li & 1) ? hu : lu;
                                const unsigned got = (unsigned)__builtin_amdgcn_mov_dpp((int)give, 0xB1, 0xF, 0xF, true);
                                const unsigned word = (li & 1) ? (got | (mine << 16)) : (mine | (got << 16));
                                *reinterpret_cast<unsigned*>(hbase + rl * rp16 + hoff) = word;
                            }
                        }
                    }
                }
            }
        };
        auto by_fmt = [&](auto act_tag) {
            if constexpr (TRAIN_EPI) { if (e.Cpre) { body(act_tag, std::integral_constant<int, 5>{}); return; } }   // (the launcher admits Cpre only beside C, without C16)
            if (e.C && e.C16) body(act_tag, std::integral_constant<int, 3>{});
            else if (e.C16) body(act_tag, std::integral_constant<int, 2>{});
            else body(act_tag, std::integral_constant<int, 1>{});
        };
        bool grad_done = false;
        if constexpr (TRAIN_EPI) {
            if (e.gradu) {                                           // (the launcher admits it with an fp32 C only and no activation)
                switch (e.gact) {
                    case FC_ACT_GELU: body(std::integral_constant<int, 16 + FC_ACT_GELU>{}, std::integral_constant<int, 1>{}); break;
                    case FC_ACT_RELU: body(std::integral_constant<int, 16 + FC_ACT_RELU>{}, std::integral_constant<int, 1>{}); break;
                    default: body(std::integral_constant<int, 16 + FC_ACT_ELU>{}, std::integral_constant<int, 1>{}); break;
                }
                grad_done = true;
            }
        }
        if (!grad_done)
        switch (e.act) {
            case FC_ACT_GELU: by_fmt(std::integral_constant<int, FC_ACT_GELU>{}); break;
            case FC_ACT_RELU: by_fmt(std::integral_constant<int, FC_ACT_RELU>{}); break;
            case FC_ACT_ELU: by_fmt(std::integral_constant<int, FC_ACT_ELU>{}); break;
            case FC_ACT_LRELU02: by_fmt(std::integral_constant<int, FC_ACT_LRELU02>{}); break;
            default: by_fmt(std::integral_constant<int, FC_ACT_NONE>{}); break;
        }
        if (omax >= 65504.0f) atomicOr(p.ovf, 1);                 // (omax stays 0 without a limb-image output)
        if constexpr (VAR == 9) {
            FC_STAMP(6)
            if (p.stamps && threadIdx.x == 0) p.stamps[(size_t)blockIdx.x * 16 + 9] = wall_clock64();
        }
    } else if constexpr (EPI == EPI_LNQ) {
        epi_lnq(p, acc, li, lh, wave_m0, wave_n0);
    } else if constexpr (EPI == EPI_SPLINE) {
        // ---- fused rational-quadratic spline coupling (forward).  The parameter layer's columns are laid out so that this
        //      128-column tile holds all 3K+1 parameters of DPT transformed dims (spline.h): the tile goes through LDS (the
        //      accumulator layout has one parameter per lane), then each thread evaluates whole splines.  Nothing of the
        //      [rows, 25*d2] parameter matrix is written to or re-read from HBM.
        static_assert(BN == 128, "spline epilogue: the column layout is built for 128-column tiles");
        constexpr int TP = BN + 1;                                   // odd pitch: lanes walk rows conflict-free
        static_assert(((size_t)BM * TP + (size_t)BM * 9) * sizeof(float) == gemm_spline_tile_bytes<BM, BN>(), "tile + <= 9 dims of log-dets, as launch_cfg reserves them");
        if (p.ablate == 2) return;                                   // (diagnostic knob 14: main loop only)
        float* tile = smem;                                          // aliases the staging buffers (all reads are behind the loop's last barrier)
        float* part = smem + BM * TP;                                // [DPT][BM] log-det terms
        if (p.ablate != 3) {                                         // (diagnostic knob 14 = 3: no parameter-tile write)
        int tpos[TN];                                                // column -> (dim, parameter) position (K = 8: spline.h's slot order)
#pragma unroll
        for (int j = 0; j < TN; ++j) tpos[j] = spline_tile_pos(wc * TN * 32 + j * 32 + li, e.spline_K);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    tile[(wr * TM * 32 + i * 32 + mfma32_row(r, lh)) * TP + tpos[j]] = acc[i][j][r];
        } else { asm volatile("" :: "v"(acc[0][0][0]), "v"(acc[TM - 1][TN - 1][15])); }
        __syncthreads();
        if constexpr (VAR == 9) FC_STAMP(4)
        if (p.ablate == 5) return;                                   // (diagnostic knob 14 = 5: main loop + parameter-tile write + barrier)
        const int K = e.spline_K, per = 3 * K + 1, DPT = BN / per;
        const int dim0 = bn * DPT;
        if (DPT == 5) {
#pragma unroll
            for (int k = 0; k < SPL_PER_THREAD; ++k) {                  // K = 8: x2 arrives from the prefetch at the top of the kernel
                const int it = tid + k * NT, row = it % BM, dl = it / BM;
                if (it < BM * DPT) {
                    float lad = 0.f;
                    if (dim0 + dl < e.d2 && m0 + row < e.rows_valid) {
                        float y;
                        if (p.ablate == 1) { y = spl_x[k] + tile[row * TP + dl * per]; lad = tile[row * TP + dl * per + 1]; }    // (diagnostic knob 14: no spline evaluation)
                        else rq_spline_fwd<8>(spl_x[k], tile + row * TP + dl * per, 1, y, lad);        // DPT == 5 <=> K == 8
                        if (p.ablate != 4) e.xbuf[(size_t)(m0 + row) * e.ldx + e.x2_col0 + dim0 + dl] = y;       // (diagnostic knob 14 = 4: no x2 store)
                        else asm volatile("" :: "v"(y));
                    }
                    part[dl * BM + row] = lad;
                }
            }
        } else {
            for (int it = tid; it < BM * DPT; it += NT) {
                const int row = it % BM, dl = it / BM;
                float lad = 0.f;
                if (dim0 + dl < e.d2 && m0 + row < e.rows_valid) {
                    float* xp = e.xbuf + (size_t)(m0 + row) * e.ldx + e.x2_col0 + dim0 + dl;
                    float y;
                    rq_any(K, *xp, tile + row * TP + dl * per, 1, false, y, lad);
                    *xp = y;
                }
                part[dl * BM + row] = lad;
            }
        }
        if constexpr (VAR == 9) FC_STAMP(5)
        __syncthreads();
        if (tid < BM) {
            float sum = 0.f;
            for (int dl = 0; dl < DPT; ++dl) sum += part[dl * BM + tid];
            e.ldj_part[(size_t)bn * e.ldj_pitch + m0 + tid] = spl_ldj + sum;      // this (tile, row) slot has one owner per launch: reproducible
        }
        if constexpr (VAR == 9) {
            FC_STAMP(6)
            if (p.stamps && threadIdx.x == 0) p.stamps[(size_t)blockIdx.x * 16 + 9] = wall_clock64();
        }
    } else {
        static_assert(EPI == EPI_LINEAR || (TN % 2 == 0), "pair-packed epilogues need an even number of column tiles");
        float lsum[TM][16];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) lsum[i][r] = 0.f;
#pragma unroll
        for (int pr = 0; pr < TN / 2; ++pr) {
            if (2 * pr + 1 < nvalid) {
                const int col_s = wave_n0 + (2 * pr) * 32 + li, col_t = col_s + 32;
                const int j = (wave_n0 / 64 + pr) * 32 + li;        // index of the transformed / noise dim
                const float bs = p.bias[col_s], bt = p.bias[col_t];
                if (j < e.d2) {
                    // The x2 operands of the whole pair block FIRST, as independent loads: read inside the element loop (`*xp = *xp * s + t`)
                    // every load sat behind the previous element's store to the same buffer -- hipcc cannot tell the rows apart -- so a lane
                    // waited out one memory latency per element, 32 in a row: 17 of an affine tile's 53 us (round 3; C4 -5 %, C3 -4 %).
                    float xv[TM][16];
                    float* xcol = nullptr;
                    float gsc = 1.0f;
                    if constexpr (EPI == EPI_AFFINE) {
                        xcol = e.xbuf + e.x2_col0 + (j < e.split ? j : e.split_pad + (j - e.split));
                        gsc = e.post_scale ? e.post_scale[j] : 1.0f;
#pragma unroll
                        for (int i = 0; i < TM; ++i)
#pragma unroll
                            for (int r = 0; r < 16; ++r)
                                xv[i][r] = xcol[(size_t)(wave_m0 + i * 32 + mfma32_row(r, lh)) * e.ldx];
                    }
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = wave_m0 + i * 32 + mfma32_row(r, lh);
                            const float u = acc[i][2 * pr][r] + bs, t = acc[i][2 * pr + 1][r] + bt;
                            if constexpr (EPI == EPI_AFFINE) {
                                // models/affine_coupling.py:23-62: s = exp(u) | (2 sigmoid(u) - 1)(1 - 1e-8) + 1 ; y2 = x2 s + t ; x2 = (y2 - t)/s
                                // (round 3: the hardware transcendentals the spline path uses, ~8 instead of ~40 VALU per pair: with e = exp(-u),
                                // (2 sigmoid(u) - 1)(1 - 1e-8) + 1 = 2 / (1 + e) in fp32 -- (float)(1 - 1e-8) IS 1.0f -- and log s = ln 2 - ln(1 + e);
                                // e = inf (u < -88.7) gives s = 0, log s = -inf like the reference's sigmoid)
                                float sc, lsc;
                                if (e.scale_fn == FC_SCALE_EXP) { sc = __builtin_amdgcn_exp2f(u * 1.4426950408889634f); lsc = __builtin_amdgcn_logf(sc) * 0.69314718055994530942f; }   // (log of the ROUNDED s, +-inf included, as the reference takes it)
                                else {
                                    const float ope = 1.0f + __builtin_amdgcn_exp2f(u * -1.4426950408889634f);
                                    sc = 2.0f * __builtin_amdgcn_rcpf(ope);
                                    lsc = (1.0f - __builtin_amdgcn_logf(ope)) * 0.69314718055994530942f;
                                }
                                const float g = gsc;
                                float* xp = xcol + (size_t)row * e.ldx;
                                if (e.inverse) *xp = (xv[i][r] - t) / (sc * g);
                                else { *xp = xv[i][r] * (sc * g) + t; lsum[i][r] += lsc; }
                            } else if constexpr (EPI == EPI_AUGMENT) {
                                // models/augmenter.py:49-63 + distributions.py:128-153: z2 = mu + eps*sigma, ldj = -log N(z2; mu, sigma)
                                float sigma = expf(t);
                                if (e.clamp > 0.f) sigma = fminf(sigma, e.clamp);
                                const float ev = row < e.rows_valid ? e.eps[(size_t)row * e.d2 + j] : 0.f;
                                float z = u + ev * sigma;
                                const float dz = z - u;
                                const float lp = -(dz * dz) / (2.0f * sigma * sigma) - logf(sigma) - 0.91893853320467274178f;
                                if (e.val_scale) z = z / e.val_scale[j] + e.val_shift[j];     // CIF Slice.inverse: undo the ActNorm of the z2 part
                                const int idx = e.d_in + j;
                                const int col = idx < e.d1 ? idx : e.d1_pad + (idx - e.d1);
                                e.xbuf[(size_t)row * e.ldx + col] = z;
                                if (!e.inverse) lsum[i][r] -= lp;
                            } else {
                                // models/slice.py:31-44 + distributions.py:140-142: ldj = +log N(x2; mu(z), sigma(z))
                                float sigma = expf(t);
                                if (e.clamp > 0.f) sigma = fminf(sigma, e.clamp);
                                float v = e.val[(size_t)row * e.ldval + j];
                                if (e.val_scale) v = (v - e.val_shift[j]) * e.val_scale[j];
                                const float dz = v - u;
                                lsum[i][r] += -(dz * dz) / (2.0f * sigma * sigma) - logf(sigma) - 0.91893853320467274178f;
                            }
                        }
                    }
                }
            }
        }
        if (e.inverse) return;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float tot = half_wave_sum(lsum[i][r]);
                const int row = wave_m0 + i * 32 + mfma32_row(r, lh);
                if (li == 0 && row < e.rows_valid) {
                    if (WN > 1 || BN < 320) e.ldj_part[(size_t)(bn * WN + wc) * e.ldj_pitch + row] += tot;     // own slot: reproducible
                    else if (p.nbn * WN > 1) atomicAdd(e.logprob + row, tot);
                    else e.logprob[row] += tot;
                }
            }
        }
    }
}
// VAR 11, the persistent fused spline kernel (gemm_spline_persistent.hip)
template <>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void gemm_f32_kernel<128, 128, 4, 1, EPI_SPLINE, 11>(const GemmParams p);

template <int BM, int BN, int WM, int WN, int EPI, int VAR = 2>
void launch_cfg(const GemmParams& p, hipStream_t s) {
    constexpr size_t lds = gemm_lds_bytes<BM, BN, EPI, VAR>();
    GemmParams q = p;
    q.nbn = (p.N_pad + BN - 1) / BN;
    q.col_group = 0;
    if ((size_t)p.N_pad * p.K_pad * sizeof(float) > (size_t)(3u << 19) && q.nbm % 8 == 0 && q.nbn > g_knobs.gemm_colgroup && g_knobs.gemm_colgroup > 0)
        q.col_group = g_knobs.gemm_colgroup;
    q.stamps = nullptr;
    if constexpr ((EPI == EPI_SPLINE || EPI == EPI_LINEAR) && (VAR == 9 || VAR == 11)) {
        if (g_knobs.stamps == (EPI == EPI_SPLINE ? 1 : 2)) {                  // stamps (knob 20): 1 = the fused spline launches, 2 = the limb-chained Linear launches
            q.stamps = gemm_stamp_buffer((size_t)q.nbm * q.nbn * 16);
        }
    }
    char name[96];
    snprintf(name, sizeof name, "void fc::gemm_f32_kernel<%d, %d, %d, %d, %d, %d>(fc::GemmParams)", BM, BN, WM, WN, EPI, VAR);
    int grid = q.nbm * q.nbn;
    if constexpr (VAR == 11) {                                          // persistent: two workgroups per CU, a multiple of 8 (XCD order)
        static PerDeviceOnce slots_once;
        const int slots = slots_once.run([](int dev) {
            int cus = 0;
            FC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
            const int n = (2 * cus) & ~7;
            return n < 8 ? 8 : n;
        });
        if (grid > slots) grid = slots;
    }
    launch_kernel<gemm_f32_kernel<BM, BN, WM, WN, EPI, VAR>, (int)lds>(name, p.e.flops_hint, 0.0, dim3(grid), dim3(WM * WN * 64), lds, s, q);
}

}  // namespace fc
