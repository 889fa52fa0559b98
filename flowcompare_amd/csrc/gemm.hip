// The GEMM of the flow on the CDNA4 matrix cores, with fused epilogues.
//
//   C[rows, N_pad] = epilogue( sum_seg A_seg[rows, k_seg] @ W[N_pad, K_pad]^T )
//
// Every Linear of the flow (coupling MLPs, q/kv projections, the folded ActNorm+LinearLU matrix, DGCNN / PAConv 1x1
// convolutions) goes through gemm_f32_kernel; operands and results are fp32 in memory, the products run in one of the
// main loops selected by the template parameter VAR:
//   VAR 5  split-fp16, the default: each operand as two fp16 limbs (hi + lo'/2048, 2^-24 relative), 3 v_mfma_f32_32x32x16_f16
//          per product block, main and cross-product fp32 accumulators; needs the caller's Fp16Guard scope (|x| < 65504);
//   VAR 3  split-bf16: three bf16 limbs, 6 MFMAs per block, unbounded range -- the pass a guarded call is repeated with;
//   VAR 2  fp32-input MFMA (v_mfma_f32_32x32x2_f32, an exact fmaf chain): the first build's loop, kept for A/B and tests;
//   VAR 9  split-fp16 with A as the limb image its producer wrote (limb-chained layers): both operands reach LDS by DMA;
//   VAR 11 the fused spline layer (K = 8) as a persistent transposed LDS-DMA GEMM, splines evaluated from the accumulators.
// (The numbers of the variants that lost an A/B and were removed -- 0, 1, 6, 7, 8, 10 -- are not reused: profiles and DESIGN.md
// section 6 quote kernels by their template arguments.)
// Epilogues (EPI): LINEAR (bias, rank-1 extra-context term, residual, activation), SPLINE (forward rational-quadratic spline
// coupling on the tile the workgroup just produced), AFFINE / AUGMENT / SLICE (pair-packed [first 32 | second 32] columns).
//
// Layout: both operands are K-contiguous in memory (activations [rows][K], weights [N][K] exactly like torch.nn.Linear.weight;
// limb images [N][K/16][limb][16]), so one ds_read_b128 per lane is one MFMA operand.  Global -> LDS goes through registers
// (split loops: two-deep prefetch, whole-vector staging values, double-buffered LDS rows with a 16-byte pad).
// Shipped tile for the split-fp16 loop: 128x128 on eight waves of 32x64 (118 VGPRs, 4 waves per SIMD).
//
// Files: gemm_kernel.h (parameters, tile order, LDS sizes, the kernel template, launch_cfg); gemm_f32.hip / gemm_split.hip / gemm_dma.hip (the
// kernels of VAR 2 / VAR 3 and 5 / VAR 9, one translation unit each); gemm_spline_persistent.hip (VAR 11); gemm_guard.cpp (host only: guard
// scopes, deferred range check, stamp buffer); this file (launch_gemm: argument checks and tile choice).
#include "gemm_kernel.h"

namespace fc {

extern template void launch_cfg<128, 64, 4, 1, EPI_LINEAR, 2>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 2, 2, EPI_LINEAR, 2>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 320, 4, 1, EPI_LINEAR, 2>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 320, 4, 1, EPI_AFFINE, 2>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 320, 4, 1, EPI_AUGMENT, 2>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 320, 4, 1, EPI_SLICE, 2>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 64, 4, 1, EPI_LINEAR, 5>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 64, 4, 1, EPI_LINEAR, 3>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 4, 2, EPI_LINEAR, 5>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 2, 2, EPI_LINEAR, 3>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 320, 4, 1, EPI_LINEAR, 3>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 4, 2, EPI_LNQ, 5>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 4, 2, EPI_SPLINE, 5>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 2, 2, EPI_SPLINE, 3>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 4, 2, EPI_AFFINE, 5>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 4, 2, EPI_AUGMENT, 5>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 4, 2, EPI_SLICE, 5>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 320, 4, 1, EPI_AFFINE, 3>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 320, 4, 1, EPI_AUGMENT, 3>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 320, 4, 1, EPI_SLICE, 3>(const GemmParams&, hipStream_t);
extern template void launch_cfg<64, 64, 2, 2, EPI_LINEAR, 9>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 2, 2, EPI_LINEAR, 9>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 2, 2, EPI_SPLINE, 9>(const GemmParams&, hipStream_t);
extern template void launch_cfg<64, 64, 2, 1, EPI_AFFINE, 9>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 2, 2, EPI_AFFINE, 9>(const GemmParams&, hipStream_t);
extern template void launch_cfg<128, 128, 4, 1, EPI_SPLINE, 11>(const GemmParams&, hipStream_t);

bool gemm_spline_wide_on() { return g_knobs.spline_kernel == 5 && g_knobs.gemm_variant == 5 && g_knobs.fused_spline && g_knobs.limb_chain && g_knobs.spline_ablate != 3 && g_knobs.spline_ablate != 4 && g_knobs.spline_ablate != 5; }

static void launch_gemm_impl(const PackedLinear& L, const ASeg* segs, int rows_alloc, const GemmEpi& e_in, int epi_kind, hipStream_t s);
void launch_gemm(const PackedLinear& L, const ASeg* segs, int rows_alloc, const GemmEpi& e_in, int epi_kind, hipStream_t s) {
    static const bool trace = getenv("FC_FLAG_TRACE") != nullptr;      // diagnostic: which launch raises the split-fp16 range flag
    int before = 0, after = 0;
    if (trace && gemm_scope_flag()) { FC_HIP(hipStreamSynchronize(s)); FC_HIP(hipMemcpy(&before, gemm_scope_flag(), 4, hipMemcpyDeviceToHost)); }
    launch_gemm_impl(L, segs, rows_alloc, e_in, epi_kind, s);
    if (trace && gemm_scope_flag()) {
        FC_HIP(hipStreamSynchronize(s)); FC_HIP(hipMemcpy(&after, gemm_scope_flag(), 4, hipMemcpyDeviceToHost));
        if (after != before) fprintf(stderr, "[flag trace] launch_gemm epi %d rows %d N %d K %d c16 %d (scale %g) a16 %d: flag %d -> %d\n", epi_kind, rows_alloc, L.N_pad, L.K_pad, e_in.C16 != nullptr,
                                     e_in.c16_scale, e_in.A16 != nullptr, before, after);
    }
}
static void launch_gemm_impl(const PackedLinear& L, const ASeg* segs, int rows_alloc, const GemmEpi& e_in, int epi_kind, hipStream_t s) {
    if (rows_alloc % ROW_PAD != 0) throw Error(FC_ERR_INVALID, "launch_gemm: rows must be padded to ROW_PAD");
    if (L.K_pad % 32 != 0 || L.N_pad % 32 != 0 || L.nseg < 1 || L.nseg > 3) throw Error(FC_ERR_INVALID, "launch_gemm: bad packing");
    GemmParams p{};
    int kt = 0;
    for (int i = 0; i < 3; ++i) {
        p.A[i] = i < L.nseg ? segs[i].ptr : nullptr;
        p.lda[i] = i < L.nseg ? segs[i].lda : 0;
        p.kt[i] = i < L.nseg ? L.seg_k[i] / 32 : 0;
        if (i < L.nseg && (L.seg_k[i] % 32 != 0 || segs[i].lda % 4 != 0 || ((uintptr_t)segs[i].ptr & 15)))
            throw Error(FC_ERR_INVALID, "launch_gemm: A segment must be 16-byte aligned with a 32-multiple width");
        kt += p.kt[i];
    }
    if (kt * 32 != L.K_pad) throw Error(FC_ERR_INVALID, "launch_gemm: segment widths do not add up to K_pad");
    if (L.n_alloc < round_up(L.N_pad, gemm_bn(L.N_pad, epi_kind != EPI_LINEAR && epi_kind != EPI_SPLINE && epi_kind != EPI_LNQ)) || L.n_alloc < round_up(L.N_pad, 128))
        throw Error(FC_ERR_INVALID, "launch_gemm: W is not zero-padded to the column-tile grid (PackedLinear.n_alloc)");
    p.KT = kt;
    GemmEpi e = e_in;
    e.flops_hint = 2.0 * (double)(e.rows_valid > 0 ? e.rows_valid : rows_alloc) * (double)(L.n_true ? L.n_true : L.N_pad) *
                   (double)(L.k_true ? L.k_true : L.K_pad);
    p.W = L.W; p.W3 = L.W3; p.W2 = L.W2; p.ovf = gemm_scope_flag(); p.K_pad = L.K_pad; p.bias = L.bias; p.colvec = L.colvec; p.N_pad = L.N_pad;
    p.e = e;
    p.ablate = g_knobs.spline_ablate;
    const bool split = (g_knobs.gemm_variant == 3 || g_knobs.gemm_variant == 5) && L.W3 != nullptr;
    const bool f16 = g_knobs.gemm_variant == 5 && L.W2 != nullptr && gemm_scope_flag() != nullptr;
    if (epi_kind == EPI_LINEAR) {
        if ((!e.C && !e.C16) || (e.C && e.ldc < L.N_pad)) throw Error(FC_ERR_INVALID, "launch_gemm: output pitch smaller than N_pad");
        if ((e.gradu || e.Cpre) && e.A16) throw Error(FC_ERR_INVALID, "launch_gemm: the training epilogues exist on the fp32-A loops only");
        if (e.gradu && (!e.C || e.C16 || e.Cpre || e.act != FC_ACT_NONE || e.ldgu < L.N_pad || (e.gact != FC_ACT_GELU && e.gact != FC_ACT_RELU && e.gact != FC_ACT_ELU)))
            throw Error(FC_ERR_INVALID, "launch_gemm: an activation-gradient epilogue goes with an fp32 C, no activation, and GELU / RELU / ELU");
        if (e.Cpre && (!e.C || e.C16)) throw Error(FC_ERR_INVALID, "launch_gemm: a pre-activation output goes with an fp32 C and no limb image");
        if (e.C16 && !(f16 && L.N_pad > 64 && L.N_pad % 16 == 0))
            throw Error(FC_ERR_UNSUPPORTED, "launch_gemm: limb-image output exists on the eight-wave split-fp16 tile only");
        if (e.a16_scale != 0.f) throw Error(FC_ERR_INVALID, "launch_gemm: a Linear layer takes no one-accumulator activation image (only the fused spline layer reads that form)");
        if (e.A16) {
            // A arrives as the limb image of the producing layer (limb-chained MLP): the copy-only main loops
            if (!(f16 && L.nseg == 1 && L.N_pad > 64 && L.n_alloc >= round_up(L.N_pad, 128)))
                throw Error(FC_ERR_UNSUPPORTED, "launch_gemm: a limb-image A operand needs the split-fp16 loop, one segment and N > 64");
            if (g_knobs.small_tiles && (rows_alloc / 128) * ((L.N_pad + 127) / 128) <= 256 && L.N_pad % 64 == 0) {
                // fewer 128x128 tiles than workgroup slots (C1: 2 x 1024 points = 16 row tiles): four times as many 64x64 tiles, each a
                // quarter of the MFMA work per k step -- the launch is bound by one workgroup's k loop, not by throughput
                p.nbm = rows_alloc / 64;
                launch_cfg<64, 64, 2, 2, EPI_LINEAR, 9>(p, s);
            }
            else { p.nbm = rows_alloc / 128; launch_cfg<128, 128, 2, 2, EPI_LINEAR, 9>(p, s); }
        } else if (L.N_pad <= 64 || (f16 && g_knobs.small_tiles && !e.C16 && (rows_alloc / 128) * ((L.N_pad + 127) / 128) <= 128 && L.n_alloc >= round_up(L.N_pad, 64))) {
            // (64-wide layers; and fp32-A launches with at most 128 tiles of 128x128: twice as many 128x64 tiles)
            p.nbm = rows_alloc / 128;
            if (f16) launch_cfg<128, 64, 4, 1, EPI_LINEAR, 5>(p, s);
            else if (split) launch_cfg<128, 64, 4, 1, EPI_LINEAR, 3>(p, s);
            else launch_cfg<128, 64, 4, 1, EPI_LINEAR>(p, s);
        } else if (L.N_pad % 128 == 0 || L.N_pad > 320 || ((split || f16) && L.n_alloc >= round_up(L.N_pad, 128))) {
            // (with the split-bf16 loop two co-resident 128x128 workgroups beat the one-wave-per-SIMD 128x320 tile even at N = 320)
            // Default for the split-fp16 loop: 128x128 tile on EIGHT waves of 32x64 (64 accumulator registers per lane instead of
            // 128 -> 118 VGPRs -> 4 waves per SIMD instead of 2): +4 ... +19 % over four waves of 64x64 on every layer shape, and
            // better than the 8-wave 256x128 tile on the wide layers
            p.nbm = rows_alloc / 128;
            if (f16) launch_cfg<128, 128, 4, 2, EPI_LINEAR, 5>(p, s);
            else if (split) launch_cfg<128, 128, 2, 2, EPI_LINEAR, 3>(p, s);
            else launch_cfg<128, 128, 2, 2, EPI_LINEAR, 2>(p, s);
        } else {
            p.nbm = rows_alloc / 128;
            if (split) launch_cfg<128, 320, 4, 1, EPI_LINEAR, 3>(p, s); else launch_cfg<128, 320, 4, 1, EPI_LINEAR>(p, s);
        }
    } else if (epi_kind == EPI_LNQ) {
        if (!f16) throw Error(FC_ERR_UNSUPPORTED, "launch_gemm: the LayerNorm -> q fold runs on the eight-wave split-fp16 tile only");
        if (!e.C || !e.ldj_part || e.d2 % 64 != 0 || L.N_pad != e.d2 + 64 || e.ldc < 64 || e.ldj_pitch < (size_t)rows_alloc || !L.bias)
            throw Error(FC_ERR_INVALID, "launch_gemm: bad LayerNorm -> q fold arguments");
        p.nbm = rows_alloc / 128;
        if (e.A16) throw Error(FC_ERR_UNSUPPORTED, "launch_gemm: the LayerNorm -> q fold takes an fp32 A panel");
        launch_cfg<128, 128, 4, 2, EPI_LNQ, 5>(p, s);
    } else if (epi_kind == EPI_SPLINE) {
        const int K = e.spline_K;
        if (!split) throw Error(FC_ERR_UNSUPPORTED, "launch_gemm: the fused spline epilogue exists for the split GEMM loops only");
        if (!spline_bins_ok(K) || L.N_pad != spline_ncols(e.d2, K) || !e.xbuf || !e.ldj_part || e.ldj_pitch < (size_t)rows_alloc)
            throw Error(FC_ERR_INVALID, "launch_gemm: bad fused-spline arguments (layout of spline.h, per-tile log-det buffer)");
        p.nbm = rows_alloc / 128;
        if (e.a16_scale != 0.f && !(f16 && e.A16)) throw Error(FC_ERR_INVALID, "launch_gemm: a one-accumulator activation image outside the split-fp16 guard scope");
        if (f16 && e.A16) {
            if (L.nseg != 1) throw Error(FC_ERR_INVALID, "launch_gemm: a limb-image A operand must be the only segment");
            if (L.n_alloc < round_up(L.N_pad, 128)) throw Error(FC_ERR_INVALID, "launch_gemm: fused spline layer not padded to the 128-column tile grid");
            if (e.a16_scale != 0.f) {                                   // the one-accumulator image: only spline_wide.hip reads it
                if (!(g_knobs.spline_kernel == 5 && spline_wide_eligible(L, K))) throw Error(FC_ERR_INVALID, "launch_gemm: a one-accumulator activation image needs the wide fused spline kernel (spline_kernel, knob 13, = 5)");
                launch_spline_wide(L, p.e, rows_alloc, s);
            }
            else if (g_knobs.spline_kernel != 2 && K == 8 && L.bias) launch_cfg<128, 128, 4, 1, EPI_SPLINE, 11>(p, s);      // (spline_kernel, knob 13, = 4; 5 where the wide kernel does not apply)
            else launch_cfg<128, 128, 2, 2, EPI_SPLINE, 9>(p, s);      // (4 and 16 bins, knob 13 = 2: the LDS-tile epilogue on the four-wave DMA tile)
        }
        else if (f16) launch_cfg<128, 128, 4, 2, EPI_SPLINE, 5>(p, s);
        else launch_cfg<128, 128, 2, 2, EPI_SPLINE, 3>(p, s);
    } else {
        if (!L.bias || L.N_pad % 64 != 0) throw Error(FC_ERR_INVALID, "launch_gemm: pair-packed epilogue needs bias and N_pad % 64 == 0");
        p.nbm = rows_alloc / 128;
        // forward direction inside a guard scope: 128x128 tile on eight waves with the split-fp16 loop (a wave's 64 columns are one
        // [first 32 | second 32] pair block); log-dets go to the caller's slot buffer.  Otherwise (inverse, bf16-limb fallback
        // pass, fp32 variants): the 128x320 tile whose workgroup owns whole rows.
        if (e.A16 && !(epi_kind == EPI_AFFINE && f16 && e.ldj_part && !e.inverse && L.nseg == 1 && L.n_alloc >= round_up(L.N_pad, 128)))
            throw Error(FC_ERR_UNSUPPORTED, "launch_gemm: a limb-image A operand in a pair-packed epilogue exists for the forward affine coupling only");
        if (f16 && e.ldj_part && !e.inverse) {
            if (e.ldj_pitch < (size_t)rows_alloc) throw Error(FC_ERR_INVALID, "launch_gemm: log-det slot pitch smaller than the row count");
            if (e.A16 && g_knobs.small_tiles && (rows_alloc / 128) * ((L.N_pad + 127) / 128) <= 256) { p.nbm = rows_alloc / 64; launch_cfg<64, 64, 2, 1, EPI_AFFINE, 9>(p, s); }   // (small launch: 64x64 tiles, see EPI_LINEAR)
            else if (e.A16) launch_cfg<128, 128, 2, 2, EPI_AFFINE, 9>(p, s);       // limb-chained MLP: copy-only LDS-DMA loop (a wave's 64 columns = one pair block)
            else if (epi_kind == EPI_AFFINE) launch_cfg<128, 128, 4, 2, EPI_AFFINE, 5>(p, s);
            else if (epi_kind == EPI_AUGMENT) launch_cfg<128, 128, 4, 2, EPI_AUGMENT, 5>(p, s);
            else launch_cfg<128, 128, 4, 2, EPI_SLICE, 5>(p, s);
        }
        else if (epi_kind == EPI_AFFINE) { if (split) launch_cfg<128, 320, 4, 1, EPI_AFFINE, 3>(p, s); else launch_cfg<128, 320, 4, 1, EPI_AFFINE>(p, s); }
        else if (epi_kind == EPI_AUGMENT) { if (split) launch_cfg<128, 320, 4, 1, EPI_AUGMENT, 3>(p, s); else launch_cfg<128, 320, 4, 1, EPI_AUGMENT>(p, s); }
        else { if (split) launch_cfg<128, 320, 4, 1, EPI_SLICE, 3>(p, s); else launch_cfg<128, 320, 4, 1, EPI_SLICE>(p, s); }
    }
}

}  // namespace fc
