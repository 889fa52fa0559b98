// The fused spline parameter layer, round 4: a PERSISTENT 256 x 256 workgroup tile on v_mfma_f32_16x16x32_f16 with ONE accumulator per output.
//
//   params[rows, 3750] = h[rows, 512] W^T + b ;  y2, log-det = RQ-spline(x2; params)      (models/spline_coupling.py:187-210, models/nets.py:19-30)
//
// Why another kernel (profiles/micro/wide_gemm_probe.hip measured the structure first): the shipped VAR 11 loop
// (gemm.hip: 128 x 128 tile, 32x32x16 MFMAs, main + cross-product accumulator sets) sat at 48 % matrix-pipe busy at 1.94 GHz for two rounds
// whatever the loop order.  Three things change here, each measured in the probe:
//   * ONE accumulator set.  The low limb is stored UNSCALED, lo = rn16(x - hi) (fp16 subnormals are honoured by the MFMA at full rate), so the
//     three limb products hi.hi + lo.hi + hi.lo land at their true scale in one fp32 accumulator.  Operands are pre-scaled by exact powers of
//     two so that lo stays a normal fp16 number for every value that matters: activations by kOneAccActScale (their producer's epilogue
//     writes the image that way), weights per layer so that max |w| lands in [2^14, 2^15) (spline_wide_attach); the product is scaled back
//     inside the spline's own first fma.  Error against fp64 at K = 512: 6.9e-8 mean / 7.1e-7 max on unit-scale outputs, below the fp32 fmaf
//     chain (1.05e-7 / 1.24e-6) at all three weight scales of the probe (tests/test_gpu_ops.py::test_one_accumulator_limb_form...).
//   * Half the accumulator registers pay for a 64-point x 128-parameter WAVE tile and a 256 x 256 workgroup tile: half the LDS-DMA bytes and
//     0.6 of the LDS fragment reads per MFMA of VAR 11.
//   * The 16x16x32 MFMA shape: the chip holds a higher clock on it (MI355X_MICROARCH.md, DVFS give-back item 7): main loop alone 0.50 ms
//     against 0.60-0.62 ms for the same tile on 32x32x16, same box.
// Structure (the guide's 8-phase GEMM template, cdna_hip_programming.md section 5): eight waves = 4 point blocks of 64 x 2 parameter tiles of
// 128; waves w and w + 4 share a SIMD and belong to different GROUPS; a k32 step is four phases {LOAD: fragment reads + DMA issue | barrier |
// 24 MFMAs | barrier} and group 1 runs ONE barrier behind group 0, so that on every SIMD one wave multiplies while its partner loads.
// Two 64 KB LDS stages (k32 of 256 point rows + 256 weight rows), LDS-DMA pieces of 8 rows x 128 B with the XOR swizzle on the source
// address, one continuous stream across the workgroup's tiles, bias (pre-scaled) and the x2 / log-det operands of the next tile fetched
// during the last k step.
// Epilogue in registers: with the weights as the MFMA's A operand a lane of row kq = lane >> 4 holds, for the point lane & 15 of each of
// the wave's four 16-point blocks, the 32 parameters "slot s" = 4 (16-parameter block) + register.  The layer's columns are packed so that
// slots 0..24 of row kq are ALL 25 parameters of transformed dim kq of the tile and slots 25..31 a part of dim 4 (7 + 6 + 6 + 6): four
// whole-wave evaluations (every lane busy: 16 points x 4 dims) and a fifth in which row kq takes dim 4 of point block kq after a 4 x 4
// transpose of those seven registers across the rows (v_permlane16_swap + v_permlane32_swap, one swap per register).  64 points x 5 dims =
// 5 full wave evaluations (VAR 11: 6 for the same points, one half empty).
// Shipped form of the spline layer (spline_fold, knob 34, = 1, read at fc_flow_create): the image is FOLDED to the 22 parameters per dim that carry
// information (softmax's shift invariance removes width / height logit 7, derivative logit 8 is read for no bin: spline_wide_src_col_folded,
// spline.h rq_spline_fwd_regs_folded), 22 + a 6 + 6 + 6 + 4 share of dim 4 = 28 slots per lane row = SEVEN 16-parameter blocks: a 64 x 112 wave
// tile, a 256 x 224 workgroup tile, 84 instead of 96 MFMAs per wave and k step in a kernel bound by the MFMAs it issues.
#include "common.h"
#include "activations.h"
#include "spline.h"
#include "launch.h"
#include <cstdio>
#include <cstdlib>

namespace fc {

struct SplineWideParams {
    const unsigned short* A16;   // [rows][KT][64] fp16: the activation image, one-accumulator form (pre-scaled by kOneAccActScale, lo unscaled)
    const unsigned short* W1;    // [nbn * 256][KT][64] fp16: the weight image in this kernel's column order, pre-scaled by 2^w1_exp
    const float* bias1;          // [nbn * 256] bias in the same order, times kOneAccActScale * 2^w1_exp
    float* xbuf; int ldx; int x2_col0; int d2; int rows_valid;
    float* ldj_part; size_t ldj_pitch;
    int KT;                      // k32 steps (even)
    int nbm, nbn;                // 256-row tiles, 256-column tiles (= pairs of 128-column spline tiles)
    int ntile128;                // 128-column spline tiles that exist (the last pair may be half empty)
    int col_group;
    float out_scale;             // 1 / (kOneAccActScale * 2^w1_exp)
    int ablate;                  // diagnostic spline_ablate (knob 14): 1 no spline evaluation, 2 main loop only (results invalid)
    int* ovf;                    // split-fp16 range flag (common.h Fp16Guard; EPI 3)
    // EPI 2 (plain product, fc_debug_one_acc_gemm_f32: the one-accumulator limb form by itself, for the accuracy test)
    float* C; int ldc;
    // EPI 3 (training Linear, csrc/train_linear.hip): the point operand is an fp32 PANEL [rows][lda] that is split into limbs after its LDS read
    // (a k32 step of a row is 128 bytes either way), scaled by a_scale or, for gradients, per row so that the row's maximum lands in
    // [2^13, 2^14) (row_absmax: max |a| of every row, written by the producing kernel); C = (acc / scale (+ addend)) (* act'(gradu))
    const float* A32; int lda;
    const float* row_absmax;
    float a_scale;
    const float* addend; const float* gradu; int ldgu; int gact;
    int n_cols;                  // columns of C that exist (a multiple of 4; the last 256-column tile may be partly empty)
};

// column of the kernel's tile order: row kq = (c >> 2) & 3 of 16-parameter block jb = c >> 4, register r = c & 3 -> slot s = 4 jb + r
//   s < 25: parameter s of the tile's dim kq;  s >= 25: parameter base(kq) + s - 25 of dim 4 (kq = 0: 0..6, 1: 7..12, 2: 13..18, 3: 19..24)
// returns the column of the SAME tile in spline.h's order (what PackedLinear.W holds), or -1 for the three unused slots
__host__ __device__ inline int spline_wide_src_col(int c) {
    const int jb = c >> 4, kq = (c >> 2) & 3, r = c & 3, s = 4 * jb + r;
    if (s < 25) return spline_col(kq, s, 8);
    const int base = kq == 0 ? 0 : 1 + 6 * kq, cnt = kq == 0 ? 7 : 6, i = s - 25;
    return i < cnt ? spline_col(4, base + i, 8) : -1;
}

// The FOLDED tile order (spline_fold, knob 34, shipped): 22 informative parameters per dim, [7 width | 7 height | 8 derivative] (spline.h
// rq_spline_fwd_regs_folded), on a wave tile of 7 blocks of 16 = 112 columns.  Column c as above; slot s = 4 jb + r < 28 of row kq:
//   s < 22: folded parameter s of the tile's dim kq;  s >= 22: folded parameter 6 kq + s - 22 of dim 4 (rows 0..2 carry 6, row 3 carries 4:
//   its last two slots are spare)
// returns the column of the same tile in spline.h's order that holds the parameter, or -1 for a spare slot; *sub receives the column that is
// SUBTRACTED from it (width / height logit 7 of the same dim), or -1 for a derivative logit
__host__ __device__ inline int spline_wide_src_col_folded(int c, int* sub) {
    const int jb = c >> 4, kq = (c >> 2) & 3, r = c & 3, s = 4 * jb + r;
    const int dim = s < 22 ? kq : 4, q = s < 22 ? s : 6 * kq + s - 22;
    *sub = -1;
    if (q >= 22) return -1;
    if (q < 14) *sub = spline_col(dim, q < 7 ? 7 : 15, 8);
    return spline_col(dim, q < 7 ? q : q < 14 ? q + 1 : q + 2, 8);
}

// ---------------------------------------------------------------- weight image + bias in the kernel's order (fc_flow_create)
__global__ __launch_bounds__(256) void spline_wide_image_kernel(const float* __restrict__ W, const float* __restrict__ bias, int n_src, int K_pad, float wscale,
                                                                float bscale, unsigned short* __restrict__ W1, float* __restrict__ bias1, size_t n, int permute) {
    // permute: 0 natural row order, 1 the 128-column tile order, 2 the folded 112-column order.  The fold W_i - W_7 is taken in double from the
    // fp32 matrix, which holds the checkpoint's values exactly: the bits of a double-precision fold of the checkpoint tensors rounded to fp32.
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const size_t row = t / K_pad;
    const int k = (int)(t - row * K_pad);
    const int tw = permute == 2 ? 112 : 128;
    const int tile = (int)(row / tw), c = (int)(row - (size_t)tile * tw);
    int sub = -1;
    const int sc = permute == 2 ? spline_wide_src_col_folded(c, &sub) : permute ? spline_wide_src_col(c) : c;
    const int srow = tile * 128 + sc, subrow = tile * 128 + sub;
    const bool live = sc >= 0 && srow < n_src;
    float x = 0.f, bv = 0.f;
    if (live) {
        x = W[(size_t)srow * K_pad + k];
        bv = bias ? bias[srow] : 0.f;
        if (sub >= 0) {
            x = (float)((double)x - (double)W[(size_t)subrow * K_pad + k]);
            bv = bias ? (float)((double)bv - (double)bias[subrow]) : 0.f;
        }
        x *= wscale;
    }
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)(x - (float)h);
    const size_t blk = row * (K_pad / 16) + k / 16;
    W1[blk * 32 + (k & 15)] = __builtin_bit_cast(unsigned short, h);
    W1[blk * 32 + 16 + (k & 15)] = __builtin_bit_cast(unsigned short, l);
    if (k == 0 && bias1) bias1[row] = bv * bscale;
}

// sum over the four rows of 16 lanes, result in every row (fixed order: (r0 + r1) + (r2 + r3))
__device__ __forceinline__ float sw_row_sum(float v) {
    float a = v, b = v;
    swap16(a, b);
    float c = a + b, d = c;
    swap32(c, d);
    return c + d;
}

// eight fp32 values (k = 8 kq .. 8 kq + 7 of one point) -> the hi / lo operand fragments of the one-accumulator form, x s = hi + lo with s an
// exact power of two; amax collects max |x s| (the caller turns it into the range flag).  Four instructions per pair of values + the running maximum (measured issue
// costs on gfx950, profiles/micro/valu_rate_probe.hip: v_pk_mul_f32 6.6, v_cvt_pk_f16_f32 8.1, v_fma_mix_f32 8.4 cycles per wave; the all-mix
// form of activations.h limb_split2s is six at 8.4 - 9.3).
typedef float sw_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void sw_split2v(sw_f32x2 x, sw_f32x2 sv, unsigned& hi, unsigned& lo, float& amax) {
    sw_f32x2 t;
    asm("v_pk_mul_f32 %0, %1, %2" : "=v"(t) : "v"(x), "v"(sv));
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(hi) : "v"(t[0]), "v"(t[1]));
    // (x s - hi is exact in fp32, so v_fma_mixlo / mixhi_f16 round it once, straight into the halves of lo: the bits of the two v_fma_mix_f32 +
    //  v_cvt_pk_f16_f32 this replaced, one instruction fewer per pair -- activations.h limb_split2u)
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(lo) : "v"(t[0]), "v"(hi));
    asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lo) : "v"(t[1]), "v"(hi));
    asm volatile("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(amax) : "v"(t[0]), "v"(t[1]));      // (volatile: pins the running maximum; left to hipcc the raw values of a k step are kept for one reduction tree and spill)
}
__device__ __forceinline__ void sw_split8(const float4& r0, const float4& r1, float sv, f16x8& hi, f16x8& lo, float& amax) {
    u32x4 h, l;
    unsigned a, b;
    const sw_f32x2 s2 = {sv, sv};
    sw_split2v(sw_f32x2{r0.x, r0.y}, s2, a, b, amax); h[0] = a; l[0] = b;
    sw_split2v(sw_f32x2{r0.z, r0.w}, s2, a, b, amax); h[1] = a; l[1] = b;
    sw_split2v(sw_f32x2{r1.x, r1.y}, s2, a, b, amax); h[2] = a; l[2] = b;
    sw_split2v(sw_f32x2{r1.z, r1.w}, s2, a, b, amax); h[3] = a; l[3] = b;
    hi = __builtin_bit_cast(f16x8, h);
    lo = __builtin_bit_cast(f16x8, l);
}

constexpr int SW_LDS = 4 * 32768 + 2 * 1024;      // two stages of (256 point rows + 256 weight rows) x 128 B, two bias buffers of 256 floats

// DMA pieces per LOAD segment of a k step, for the group that fetches the points (waves 0-3: P*) and the weights (waves 4-7: Q*); the
// lagging group must not issue in its last segment (it waits for its pieces there)
// EPI 0: the fused spline coupling; EPI 2: the plain product (debug ABI); EPI 3: a training Linear layer (same main loop, same
// one-accumulator arithmetic; the weight image in natural row order)
template <int EPI, int P0, int P1, int P2, int P3, int Q0, int Q1, int Q2, int Q3>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2)))
void spline_wide_kernel(const SplineWideParams p) {
    // NB: 16-parameter blocks of a wave tile = weight DMA pieces per fetching wave and k step.  8: the 64 x 128 wave tile (every EPI);
    // 7: the folded spline image, a 64 x 112 wave tile (EPI 0 only): 84 instead of 96 MFMAs per wave and k step, 224 weight rows per stage
    constexpr int NB = Q0 + Q1 + Q2;
    static_assert((EPI == 0 || EPI == 2 || EPI == 3) && P0 + P1 + P2 + P3 == 8 && (NB == 8 || (NB == 7 && EPI == 0)) && Q3 == 0, "eight point pieces and NB weight pieces per wave and k step");
    extern __shared__ char smc[];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, pw = wave & 3;
    const int KT = p.KT;
    constexpr bool AF32 = EPI == 3;                                      // the point operand is an fp32 panel (split into limbs in registers)
    const unsigned rowbytes = (AF32 && grp == 0) ? (unsigned)p.lda * 4u : (unsigned)KT * 128u;      // of the operand THIS wave fetches
    const int ntiles = p.nbm * p.nbn, G = gridDim.x;
    int t = blockIdx.x;
    if (t >= ntiles) return;
    float* biasbuf = reinterpret_cast<float*>(smc + 4 * 32768);          // [2][256]

    auto tile_of = [&](int b, int& bm, int& bn) {                       // XCD-aware order (gemm.hip): blocks b, b + 8, ... share an XCD
        const int xcd = b & 7, loc = b >> 3;
        if (p.col_group > 0) {
            const int rows_x = p.nbm >> 3, Gc = p.col_group;
            const int g = loc / (rows_x * Gc);
            const int rem = loc - g * rows_x * Gc;
            const int w = p.nbn - g * Gc < Gc ? p.nbn - g * Gc : Gc;
            const int r = rem / w;
            bm = xcd * rows_x + r;
            bn = g * Gc + (rem - r * w);
        } else {
            const int q = ntiles >> 3, r = ntiles & 7;
            const int L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
            bm = L / p.nbn;
            bn = L - bm * p.nbn;
        }
    };
    // LDS: [stage 0 points 32 KB | stage 1 points | stage 0 weights | stage 1 weights]; a row = 128 B = one k32 step of one point / weight row
    // = 8 chunks of 16 B, logical chunk c = 4 (k16 block) + 2 limb + (k half) at physical chunk c ^ ((row >> 1) & 7).
    // DMA piece i of this wave: point rows (wave & 3) * 64 + 8 i + (lane >> 3), weight rows (wave & 3) * 8 NB + 8 i + (lane >> 3).
    unsigned poff[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int r = pw * (grp == 0 ? 64 : 8 * NB) + par * 8 + (lane >> 3);      // (8 NB is a multiple of 8: the swizzle term still depends on the parity of i only)
        const int cl = (lane & 7) ^ ((r >> 1) & 7);
        poff[par] = (unsigned)r * rowbytes + cl * 16;
    }
    auto src_of = [&](int bm, int bn) -> const char* {
        return grp == 0 ? (AF32 ? reinterpret_cast<const char*>(p.A32) : reinterpret_cast<const char*>(p.A16)) + (size_t)bm * 256 * rowbytes
                        : reinterpret_cast<const char*>(p.W1) + (size_t)bn * (32 * NB) * rowbytes;
    };
    const int dst0 = grp == 0 ? pw * 8192 : 65536 + pw * (1024 * NB);
#define SW_DMA(SRC_, ST_, I0_, N_)                                                                                                      \
    {                                                                                                                                     \
        _Pragma("unroll") for (int i_ = (I0_); i_ < (I0_) + (N_); ++i_)                                                                 \
            lds_dma16((SRC_) + (size_t)(i_ >> 1) * 16 * rowbytes + poff[i_ & 1], smc + dst0 + (ST_) * 32768 + i_ * 1024);               \
    }
    auto bias_dma = [&](int bn, int par) {                              // 256 floats: waves 0-3, 4 bytes per lane (NB = 7: 224 in use; bias1 is padded by 32)
        if (grp == 0 && (EPI != 3 || p.bias1))
            lds_dma4(p.bias1 + bn * (32 * NB) + pw * 64 + lane, biasbuf + par * 256 + pw * 64);
    };
    // a k32 step is ONE k extent of the 16x16x32 MFMA: lane (l15, kq) supplies row l15 of a 16-row block, k quarter kq = chunks 0, 1, 4, 5 of
    // the hi limb / 2, 3, 6, 7 of the lo limb
    const int xsw = (l15 >> 1) & 7;
    int abase[2], bbase[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int c = (((kq >> 1) * 4 + q * 2 + (kq & 1)) ^ xsw) * 16;
        abase[q] = (pw * 64 + l15) * 128 + c;
        bbase[q] = 65536 + (grp * 16 * NB + l15) * 128 + c;
    }
    // EPI 3: the point rows arrive as fp32 (a k32 step of a row = 32 floats = the same 128 bytes) and are turned into the limb image IN PLACE, one
    // k step ahead of their use: lane (l15, kq) reads the eight floats k = 8 kq .. 8 kq + 7 (chunks 2 kq, 2 kq + 1) and writes their hi / lo
    // limbs to the image's chunks; wave w converts point blocks 0, 1 of its 64 rows, wave w + 4 (the other group, same rows) blocks 2, 3
    const int cbase = (pw * 64 + grp * 32 + l15) * 128;
    const int cin0 = ((2 * kq) ^ xsw) * 16, cin1 = ((2 * kq + 1) ^ xsw) * 16;
    const int cout0 = abase[0] - (pw * 64 + l15) * 128, cout1 = abase[1] - (pw * 64 + l15) * 128;
    // EPI 3: scale of this lane's four points (point (ib, l15)) and what undoes it in the epilogue
    float csc[2] = {1.f, 1.f}, amax = 0.f;                               // scales of the two point blocks this wave converts (of the tile whose data comes next)
    bool bad_row = false;
    auto row_scale = [&](int bm, int ib0, int n, float* sc) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) break;
            const int ib = ib0 + j;
            if (p.row_absmax) {
                const unsigned bits = __builtin_bit_cast(unsigned, p.row_absmax[bm * 256 + pw * 64 + ib * 16 + l15]);
                const int e = (int)((bits >> 23) & 0xffu);                       // biased exponent of the row's maximum: 2^(e - 127) <= max < 2^(e - 126)
                int se = e == 0 ? 127 : 267 - e;                                 // scale 2^(13 - (e - 127)): max lands in [2^13, 2^14)
                se = se > 254 ? 254 : se;
                bad_row |= e == 255;                                             // inf / NaN in the row: range flag
                sc[j] = __builtin_bit_cast(float, (unsigned)se << 23);
            } else sc[j] = p.a_scale;
        }
    };
    // converts this wave's two point blocks of LDS stage `st` in place (reads before writes: one wave's LDS operations execute in order)
    auto convert_stage = [&](int st) {
        char* base = smc + st * 32768 + cbase;
        const float4 a0 = *reinterpret_cast<const float4*>(base + cin0), a1 = *reinterpret_cast<const float4*>(base + cin1);
        const float4 b0 = *reinterpret_cast<const float4*>(base + 2048 + cin0), b1 = *reinterpret_cast<const float4*>(base + 2048 + cin1);
        f16x8 h0, l0, h1, l1;
        sw_split8(a0, a1, csc[0], h0, l0, amax);
        sw_split8(b0, b1, csc[1], h1, l1, amax);
        *reinterpret_cast<f16x8*>(base + cout0) = h0;
        *reinterpret_cast<f16x8*>(base + cout1) = l0;
        *reinterpret_cast<f16x8*>(base + 2048 + cout0) = h1;
        *reinterpret_cast<f16x8*>(base + 2048 + cout1) = l1;
    };
    // this lane's share of a tile's x2 operands: dim kq of point (ib, l15) for ib = 0..3, dim 4 of point (kq, l15), and that point's log-det slot
    auto load_x = [&](int bm, int bn, float (&x)[5], float& ldj) {
        const int t128 = 2 * bn + grp, dim0 = t128 * 5;
        const int row0 = bm * 256 + pw * 64 + l15;
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) {
            const int row = row0 + 16 * ib;
            x[ib] = row < p.rows_valid && dim0 + kq < p.d2 ? p.xbuf[(size_t)row * p.ldx + p.x2_col0 + dim0 + kq] : 0.f;
        }
        const int rowq = row0 + 16 * kq;
        x[4] = rowq < p.rows_valid && dim0 + 4 < p.d2 ? p.xbuf[(size_t)rowq * p.ldx + p.x2_col0 + dim0 + 4] : 0.f;
        ldj = t128 < p.ntile128 ? p.ldj_part[(size_t)t128 * p.ldj_pitch + rowq] : 0.f;
    };

    int bm, bn;
    tile_of(t, bm, bn);
    const char* src = src_of(bm, bn);
    if constexpr (NB == 8) SW_DMA(src, 0, 0, 8)
    else if (grp == 0) SW_DMA(src, 0, 0, 8)
    else SW_DMA(src, 0, 0, NB)
    bias_dma(bn, 0);
    float spl_x[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, spl_ldj = 0.f;
    if constexpr (EPI == 0) load_x(bm, bn, spl_x, spl_ldj);
    if constexpr (EPI == 3) row_scale(bm, 2 * grp, 2, csc);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (AF32) {
        convert_stage(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    if (grp == 1) __builtin_amdgcn_s_barrier();                         // the second group runs one segment behind the first

    floatx4 acc[4][NB];
    int par = 0;
    for (;;) {
        const int tn = t + G;
        const bool has_next = tn < ntiles;
        int nbm = bm, nbn = bn;
        if (has_next) tile_of(tn, nbm, nbn);
        const char* nsrc = src_of(nbm, nbn);
        float nx[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, nldj = 0.f;
        {
            // accumulators start from the (pre-scaled) bias: register r of block jb is tile column 16 jb + 4 kq + r for every point block
            const float* bb = biasbuf + par * 256 + grp * 16 * NB + 4 * kq;
            const bool has_bias = EPI != 3 || p.bias1 != nullptr;
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
                const float4 b4 = has_bias ? *reinterpret_cast<const float4*>(bb + jb * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int ib = 0; ib < 4; ++ib) { acc[ib][jb][0] = b4.x; acc[ib][jb][1] = b4.y; acc[ib][jb][2] = b4.z; acc[ib][jb][3] = b4.w; }
            }
        }
#define SW_PHASE(ST_, F_, NP_, NQ_, I0P_, I0Q_, LAST_)                                                                                   \
        {                                                                                                                                 \
            if ((F_) == 0) {                                                                                                              \
                _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                            \
                    _Pragma("unroll") for (int q = 0; q < 2; ++q)                                                                        \
                        xf[i][q] = *reinterpret_cast<const f16x8*>(smc + abase[q] + (ST_) * 32768 + i * 2048);                            \
            }                                                                                                                             \
            _Pragma("unroll") for (int jj = 0; jj < 2 && 2 * (F_) + jj < NB; ++jj)                                                       \
                _Pragma("unroll") for (int q = 0; q < 2; ++q)                                                                            \
                    wf[jj][q] = *reinterpret_cast<const f16x8*>(smc + bbase[q] + (ST_) * 32768 + (2 * (F_) + jj) * 2048);                 \
            if (grp == 0) { if ((NP_) > 0) SW_DMA(dsrc, (ST_) ^ 1, I0P_, NP_) }                                                          \
            else { if ((NQ_) > 0) SW_DMA(dsrc, (ST_) ^ 1, I0Q_, NQ_) }                                                                   \
            if constexpr (AF32) {                                        /* the NEXT k step's point rows (all of them issued in phases 0, 1): fp32 -> limb image in place */ \
                if ((F_) == 3) {                                                                                                          \
                    if (grp == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     /* own rows; the other group converts behind the next barrier */ \
                    convert_stage((ST_) ^ 1);                                                                                             \
                }                                                                                                                         \
            }                                                                                                                             \
            if ((LAST_) && grp == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                     \
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                            \
            __builtin_amdgcn_sched_barrier(0);                                                                                            \
            __builtin_amdgcn_s_barrier();                                                                                                 \
            __builtin_amdgcn_sched_barrier(0);                                                                                            \
            __builtin_amdgcn_s_setprio(1);                                                                                                \
            _Pragma("unroll") for (int pr = 0; pr < 3; ++pr)                                                                             \
                _Pragma("unroll") for (int jj = 0; jj < 2 && 2 * (F_) + jj < NB; ++jj)                                                   \
                    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                        \
                        acc[i][2 * (F_) + jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[jj][pr == 1 ? 1 : 0], xf[i][pr == 2 ? 1 : 0],  \
                                                                                       acc[i][2 * (F_) + jj], 0, 0, 0);                   \
            __builtin_amdgcn_s_setprio(0);                                                                                                \
            if ((LAST_) && grp == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                     \
            __builtin_amdgcn_sched_barrier(0);                                                                                            \
            __builtin_amdgcn_s_barrier();                                                                                                 \
            __builtin_amdgcn_sched_barrier(0);                                                                                            \
        }
#define SW_STEP(ST_)                                                                                                                      \
        {                                                                                                                                 \
            SW_PHASE(ST_, 0, P0, Q0, 0, 0, 0)                                                                                             \
            SW_PHASE(ST_, 1, P1, Q1, P0, Q0, 0)                                                                                           \
            SW_PHASE(ST_, 2, P2, Q2, P0 + P1, Q0 + Q1, 0)                                                                                 \
            SW_PHASE(ST_, 3, P3, Q3, P0 + P1 + P2, Q0 + Q1 + Q2, 1)                                                                       \
        }
        f16x8 xf[4][2], wf[2][2];
        for (int kt = 0; kt < KT; kt += 2) {
            const char* dsrc = src + (size_t)(kt + 1) * 128;
            SW_STEP(0)
            const bool lastk = kt + 2 >= KT;
            dsrc = lastk ? nsrc : src + (size_t)(kt + 2) * 128;
            if (lastk && has_next) {                                    // the stream runs on into the next tile: its bias and x2 / log-det operands too
                bias_dma(nbn, par ^ 1);
                if constexpr (EPI == 0) load_x(nbm, nbn, nx, nldj);
                if constexpr (EPI == 3) row_scale(nbm, 2 * grp, 2, csc);      // (this tile's remaining conversion is the next tile's first k step)
            }
            SW_STEP(1)
        }
        // ---------------------------------------------------------------- epilogue in registers
        // Tile boundary: group 0 has finished its last MFMA segment one barrier before group 1.  It waits that one segment out, so that BOTH
        // groups evaluate their splines in the same interval: two waves per SIMD issue VALU work at twice the rate of one (a lone wave issues
        // an instruction every 4 cycles), and the evaluation is ~1400 VALU instructions per wave and tile.  Group 1 then re-enters one barrier
        // behind group 0 again.  (First form of this kernel: group 0's evaluation beside group 1's last MFMAs, group 1's beside group 0's
        // first: the two evaluations stood in series, 0.13 of 0.63 ms per launch.)
        if (grp == 0) {
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (EPI == 3) {
            // ---- training Linear: C = (acc / scale + addend) * act'(gradu); a lane holds columns 16 jb + 4 kq + 0..3 of point (ib, l15)
            float asc[4];
            row_scale(bm, 0, 4, asc);
#pragma unroll
            for (int ib = 0; ib < 4; ++ib) {
                const size_t row = (size_t)(bm * 256 + pw * 64 + ib * 16 + l15);
                const int col0 = bn * 256 + grp * 128 + 4 * kq;
                // (a per-row scale is an exact power of two 2^(se - 127): its inverse is the exponent 254 - se)
                const float sc = p.row_absmax ? __builtin_bit_cast(float, (254u - (__builtin_bit_cast(unsigned, asc[ib]) >> 23)) << 23) * p.out_scale : p.out_scale;
#pragma unroll
                for (int jb = 0; jb < 8; ++jb) {
                    const int col = col0 + jb * 16;
                    if (col < p.n_cols) {
                        float4 v = make_float4(acc[ib][jb][0] * sc, acc[ib][jb][1] * sc, acc[ib][jb][2] * sc, acc[ib][jb][3] * sc);
                        if (p.addend) {
                            const float4 a = *reinterpret_cast<const float4*>(p.addend + row * p.ldc + col);
                            v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
                        }
                        if (p.gradu) {
                            const float4 u = *reinterpret_cast<const float4*>(p.gradu + row * p.ldgu + col);
                            v.x *= fc_gelu_grad(u.x); v.y *= fc_gelu_grad(u.y); v.z *= fc_gelu_grad(u.z); v.w *= fc_gelu_grad(u.w);      // (GELU only: launch_train_wide checks)
                        }
                        const floatx4 v4 = {v.x, v.y, v.z, v.w};
                        *reinterpret_cast<floatx4*>(p.C + row * p.ldc + col) = v4;
                    }
                }
            }
        } else
        if constexpr (EPI == 2) {
            const float os = p.out_scale;
#pragma unroll
            for (int ib = 0; ib < 4; ++ib) {
                float* cr = p.C + (size_t)(bm * 256 + pw * 64 + ib * 16 + l15) * p.ldc + bn * 256 + grp * 128 + 4 * kq;
#pragma unroll
                for (int jb = 0; jb < 8; ++jb)
                    *reinterpret_cast<float4*>(cr + jb * 16) = make_float4(acc[ib][jb][0] * os, acc[ib][jb][1] * os, acc[ib][jb][2] * os, acc[ib][jb][3] * os);
            }
        } else
        if (p.ablate != 2) {
            const float os = p.out_scale;
            const int t128 = 2 * bn + grp, dim0 = t128 * 5;
            const int row0 = bm * 256 + pw * 64 + l15, rowq = row0 + 16 * kq;
            // NB = 8: slots 25..31 (registers 1..3 of block 6, 0..3 of block 7), NB = 7: slots 22..27 (registers 2, 3 of block 5, 0..3 of block 6):
            // the parts of dim 4 -> row d gets the parts of point block d
            constexpr int S4 = NB == 8 ? 25 : 22;
#pragma unroll
            for (int s = S4; s < 4 * NB; ++s) {
                float x0 = acc[0][s >> 2][s & 3], x1 = acc[1][s >> 2][s & 3], x2 = acc[2][s >> 2][s & 3], x3 = acc[3][s >> 2][s & 3];
                swap16(x0, x1);
                swap16(x2, x3);
                swap32(x0, x2);
                swap32(x1, x3);
                acc[0][s >> 2][s & 3] = x0; acc[1][s >> 2][s & 3] = x1; acc[2][s >> 2][s & 3] = x2; acc[3][s >> 2][s & 3] = x3;
            }
            float yv[5], lv[5];
            if (p.ablate == 1) {
#pragma unroll
                for (int ib = 0; ib < 4; ++ib) { yv[ib] = spl_x[ib] + acc[ib][0][0] * os; lv[ib] = acc[ib][0][1] * os; }
                yv[4] = spl_x[4] + acc[0][6][1] * os; lv[4] = acc[1][6][1] * os;
            } else if constexpr (NB == 7) {
#pragma unroll
                for (int ib = 0; ib < 4; ++ib)
                    rq_spline_fwd_regs_folded(spl_x[ib], [&](int q) { return acc[ib][q >> 2][q & 3]; }, os, yv[ib], lv[ib]);
                // dim 4: folded parameters 6 d .. 6 d + 5 from (transposed) block d, slots 22 + i
                rq_spline_fwd_regs_folded(spl_x[4], [&](int q) {
                    const int part = q / 6, s = 22 + q % 6;
                    return acc[part][s >> 2][s & 3];
                }, os, yv[4], lv[4]);
            } else {
#pragma unroll
                for (int ib = 0; ib < 4; ++ib)
                    rq_spline_fwd_regs<8>(spl_x[ib], [&](int q) { return acc[ib][q >> 2][q & 3]; }, os, yv[ib], lv[ib]);
                // dim 4: parameters 0..6 from (transposed) block 0, 7..12 from block 1, 13..18 from block 2, 19..24 from block 3, slots 25 + i
                rq_spline_fwd_regs<8>(spl_x[4], [&](int q) {
                    const int part = q < 7 ? 0 : (q - 1) / 6, s = 25 + (q < 7 ? q : (q - 1) % 6);
                    return acc[part][s >> 2][s & 3];
                }, os, yv[4], lv[4]);
            }
            const bool dk = dim0 + kq < p.d2, d4 = dim0 + 4 < p.d2;
            float tot = 0.f;
#pragma unroll
            for (int ib = 0; ib < 4; ++ib) {
                const bool v = dk && row0 + 16 * ib < p.rows_valid;
                const float s4 = sw_row_sum(v ? lv[ib] : 0.f);             // dims 0..3 of point (ib, l15), in every row
                tot = kq == ib ? s4 : tot;
                if (v) p.xbuf[(size_t)(row0 + 16 * ib) * p.ldx + p.x2_col0 + dim0 + kq] = yv[ib];
            }
            const bool vq = rowq < p.rows_valid;
            if (vq && d4) { p.xbuf[(size_t)rowq * p.ldx + p.x2_col0 + dim0 + 4] = yv[4]; tot += lv[4]; }
            if (t128 < p.ntile128) p.ldj_part[(size_t)t128 * p.ldj_pitch + rowq] = spl_ldj + tot;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) asm volatile("" ::"v"(acc[i][j]));
        }
        if (grp == 1) {
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!has_next) break;
        t = tn; bm = nbm; bn = nbn; src = nsrc; par ^= 1;
#pragma unroll
        for (int i = 0; i < 5; ++i) spl_x[i] = nx[i];
        spl_ldj = nldj;
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();
    if constexpr (EPI == 3) { if (p.ovf && (bad_row || !(amax < 65504.0f))) atomicOr(p.ovf, 1); }      // (amax: of the scaled values; also on a NaN)
#undef SW_DMA
#undef SW_PHASE
#undef SW_STEP
}

// ---------------------------------------------------------------- host side
bool spline_wide_eligible(const PackedLinear& L, int K_bins) {
    return K_bins == 8 && L.W1 != nullptr && L.bias1 != nullptr && L.nseg == 1 && L.K_pad % 64 == 0 && L.N_pad % 128 == 0;
}

// Attaches the kernel's weight image and bias to the packed spline parameter layer (K = 8 bins; W / bias hold spline.h's column order).
// wmax = max |w| over the rows the image holds (host side, from the checkpoint tensor; fold: over the FOLDED rows, up to twice the tensor's).
// fold: the 22-parameter image on 112-column wave tiles (spline_wide_src_col_folded); W / W2 / W3 / bias stay as they are.
void spline_wide_attach(DeviceArena& arena, PackedLinear& L, float wmax, hipStream_t s, bool fold) {
    if (!L.W || !L.bias || !L.W2 || L.nseg != 1 || L.K_pad % 64 != 0 || L.N_pad % 128 != 0 || L.n_alloc < L.N_pad) return;
    if (!(wmax < 65504.0f)) return;
    int e = 0;
    if (wmax > 0.f) {
        while (ldexpf(wmax, e) >= 32768.0f) --e;
        while (ldexpf(wmax, e) < 16384.0f && e < 100) ++e;
    }
    const int rows = fold ? round_up(L.N_pad, 256) / 256 * 224 : round_up(L.N_pad, 256);      // workgroup tiles of 2 x 112 / 2 x 128 columns
    const size_t n = (size_t)rows * L.K_pad;
    L.W1 = (unsigned short*)arena.alloc_bytes(n * 2 * sizeof(unsigned short));
    L.bias1 = arena.alloc_floats((size_t)rows + (fold ? 32 : 0));      // (the kernel fetches 256 floats per workgroup tile)
    L.w1_exp = e;
    L.w1_folded = fold;
    launch_kernel<spline_wide_image_kernel>(nullptr, 0.0, 0.0, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, L.W, L.bias, L.N_pad, L.K_pad, ldexpf(1.f, e),
                                            kOneAccActScale * ldexpf(1.f, e), L.W1, L.bias1, n, fold ? 2 : 1);
}

void launch_spline_wide(const PackedLinear& L, const GemmEpi& e, int rows_alloc, hipStream_t s) {
    if (!spline_wide_eligible(L, e.spline_K) || !e.A16 || e.a16_scale != kOneAccActScale || rows_alloc % 256 != 0 || !e.xbuf || !e.ldj_part ||
        e.ldj_pitch < (size_t)rows_alloc || L.N_pad != spline_ncols(e.d2, 8))
        throw Error(FC_ERR_INVALID, "launch_spline_wide: needs the one-accumulator activation image, the attached weight image and rows padded to 256");
    SplineWideParams p{};
    p.A16 = e.A16; p.W1 = L.W1; p.bias1 = L.bias1;
    p.xbuf = e.xbuf; p.ldx = e.ldx; p.x2_col0 = e.x2_col0; p.d2 = e.d2; p.rows_valid = e.rows_valid;
    p.ldj_part = e.ldj_part; p.ldj_pitch = e.ldj_pitch;
    p.KT = L.K_pad / 32;
    p.nbm = rows_alloc / 256;
    p.ntile128 = L.N_pad / 128;
    p.nbn = (p.ntile128 + 1) / 2;
    p.col_group = (p.nbm % 8 == 0 && p.nbn > 5) ? 5 : 0;
    p.out_scale = 1.0f / (kOneAccActScale * ldexpf(1.f, L.w1_exp));
    p.ablate = g_knobs.spline_ablate;
    const int cg = g_knobs.spline_wide_colgroup;      // (knob 28)
    if (cg >= 0) p.col_group = (p.nbm % 8 == 0 && p.nbn > cg) ? cg : 0;
    static PerDeviceOnce slots_once;
    const int slots = slots_once.run([](int dev) {
        int cus = 0;
        FC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        const int n = cus & ~7;                                         // one workgroup per CU, a multiple of 8 (XCD order)
        return n < 8 ? 8 : n;
    });
    int grid = p.nbm * p.nbn;
    if (grid > slots) grid = slots;
    const double flops = 2.0 * (double)(e.rows_valid > 0 ? e.rows_valid : rows_alloc) * (double)(L.n_true ? L.n_true : L.N_pad) * (double)(L.k_true ? L.k_true : L.K_pad);
    if (L.w1_folded)      // (the weight pieces of the folded form: 2 + 3 + 2 per k step)
        launch_kernel<spline_wide_kernel<0, 2, 3, 3, 0, 2, 3, 2, 0>, SW_LDS>("void fc::spline_wide_kernel<0, 2, 3, 3, 0, 2, 3, 2, 0>(fc::SplineWideParams)", flops, 0.0,
                                                                             dim3(grid), dim3(512), SW_LDS, s, p);
    else
        launch_kernel<spline_wide_kernel<0, 2, 3, 3, 0, 2, 3, 3, 0>, SW_LDS>("void fc::spline_wide_kernel<0, 2, 3, 3, 0, 2, 3, 3, 0>(fc::SplineWideParams)", flops, 0.0,
                                                                             dim3(grid), dim3(512), SW_LDS, s, p);
}

}  // namespace fc

namespace fc {

// ---------------------------------------------------------------- EPI 2: the one-accumulator limb product by itself (debug ABI, accuracy tests)
// out[rows, N] = x[rows, K] W[N, K]^T + bias on the 256 x 256 main loop: x and W are split into one-accumulator images here (x by
// kOneAccActScale, W by the power of two that puts max |w| into [2^14, 2^15) -- wmax given by the caller), rows / N padded to 256.
namespace { struct SwTmp { void* p = nullptr; explicit SwTmp(size_t b) { FC_HIP(hipMalloc(&p, b ? b : 4)); } ~SwTmp() { (void)hipFree(p); } float* f() const { return (float*)p; } }; }
void one_acc_gemm_debug(const float* x, const float* W, const float* bias, float wmax, float* out, int rows, int N, int K, hipStream_t s) {
    if (!x || !W || !out || rows < 1 || N < 1 || K < 64 || K % 64 != 0 || N % 256 != 0 || !(wmax < 65504.0f)) throw Error(FC_ERR_INVALID, "one_acc_gemm_debug: K % 64 == 0, N % 256 == 0");
    const int rp = round_up(rows, 256);
    int e = 0;
    if (wmax > 0.f) {
        while (ldexpf(wmax, e) >= 32768.0f) --e;
        while (ldexpf(wmax, e) < 16384.0f && e < 100) ++e;
    }
    SwTmp xa((size_t)rp * K * 4), wi((size_t)N * K * 4), b1((size_t)N * 4), cp((size_t)rp * N * 4), xp((size_t)rp * K * 4);
    launch_fill(xp.f(), 0.f, (size_t)rp * K, s);
    FC_HIP(hipMemcpyAsync(xp.f(), x, (size_t)rows * K * 4, hipMemcpyDeviceToDevice, s));
    const size_t nx = (size_t)rp * K, nw = (size_t)N * K;
    launch_kernel<spline_wide_image_kernel>(nullptr, 0.0, 0.0, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, s, xp.f(), nullptr, rp, K, kOneAccActScale, 0.f,
                                            (unsigned short*)xa.p, nullptr, nx, 0);
    launch_kernel<spline_wide_image_kernel>(nullptr, 0.0, 0.0, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, W, bias, N, K, ldexpf(1.f, e), kOneAccActScale * ldexpf(1.f, e),
                                            (unsigned short*)wi.p, b1.f(), nw, 0);
    SplineWideParams p{};
    p.A16 = (const unsigned short*)xa.p; p.W1 = (const unsigned short*)wi.p; p.bias1 = b1.f();
    p.KT = K / 32; p.nbm = rp / 256; p.nbn = N / 256; p.ntile128 = N / 128;
    p.col_group = (p.nbm % 8 == 0 && p.nbn > 5) ? 5 : 0;
    p.out_scale = 1.0f / (kOneAccActScale * ldexpf(1.f, e));
    p.C = cp.f(); p.ldc = N;
    int cus = 0, dev = 0;
    FC_HIP(hipGetDevice(&dev));
    FC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    int grid = p.nbm * p.nbn;
    const int slots = (cus & ~7) < 8 ? 8 : (cus & ~7);
    if (grid > slots) grid = slots;
    launch_kernel<spline_wide_kernel<2, 2, 3, 3, 0, 2, 3, 3, 0>, SW_LDS>(nullptr, 0.0, 0.0, dim3(grid), dim3(512), SW_LDS, s, p);      // (debug entry: not profiled)
    FC_HIP(hipMemcpyAsync(out, cp.f(), (size_t)rows * N * 4, hipMemcpyDeviceToDevice, s));
    FC_HIP(hipStreamSynchronize(s));
}

}  // namespace fc

namespace fc {

// ---------------------------------------------------------------- EPI 3: the wide Linear layers of a training step (train_linear.hip)

void launch_train_wide(const TrainWideArgs& a, hipStream_t s) {
    if (!a.A || !a.W1 || !a.C || a.K_pad < 64 || a.K_pad % 64 != 0 || a.rows_pad < 256 || a.rows_pad % 256 != 0 || a.n_cols < 4 || a.n_cols % 4 != 0 ||
        a.lda < a.K_pad || a.lda % 4 != 0 || a.ldc < a.n_cols || a.ldc % 4 != 0 || (a.gradu && (a.ldgu < a.n_cols || a.ldgu % 4 != 0)) ||
        (((uintptr_t)a.A | (uintptr_t)a.C | (uintptr_t)a.addend | (uintptr_t)a.gradu) & 15) || (a.row_absmax && a.bias1) || (a.gradu && a.gact != FC_ACT_GELU))
        throw Error(FC_ERR_INVALID, "launch_train_wide: K % 64 == 0, rows % 256 == 0, 16-byte aligned panels with pitches in multiples of 4, no bias beside per-row scales, GELU as the only activation gradient");
    SplineWideParams p{};
    p.A32 = a.A; p.lda = a.lda; p.W1 = a.W1; p.bias1 = a.bias1;
    p.KT = a.K_pad / 32;
    p.nbm = a.rows_pad / 256;
    p.nbn = (a.n_cols + 255) / 256;
    p.ntile128 = (a.n_cols + 127) / 128;
    p.col_group = p.nbm % 8 == 0 ? (p.nbn > 5 ? 5 : p.nbn) : 0;
    p.row_absmax = a.row_absmax;
    p.a_scale = a.a_scale;
    p.out_scale = a.row_absmax ? ldexpf(1.f, -kTrainWideWExp) : 1.0f / (a.a_scale * ldexpf(1.f, kTrainWideWExp));
    p.C = a.C; p.ldc = a.ldc; p.addend = a.addend; p.gradu = a.gradu; p.ldgu = a.ldgu; p.gact = a.gact; p.n_cols = a.n_cols;
    p.ovf = a.ovf;
    static PerDeviceOnce slots_once;
    const int slots = slots_once.run([](int dev) {
        int cus = 0;
        FC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        const int n = cus & ~7;
        return n < 8 ? 8 : n;
    });
    int grid = p.nbm * p.nbn;
    if (grid > slots) grid = slots;
    launch_kernel<spline_wide_kernel<3, 4, 4, 0, 0, 2, 3, 3, 0>, SW_LDS>("void fc::spline_wide_kernel<3, 4, 4, 0, 0, 2, 3, 3, 0>(fc::SplineWideParams)", a.flops, 0.0,
                                                                         dim3(grid), dim3(512), SW_LDS, s, p);
}

}  // namespace fc
