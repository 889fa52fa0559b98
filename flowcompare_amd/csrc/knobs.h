// The kernel-choice knobs: the one list of record.  A knob selects among kernel variants that all stay in the library because a test pins
// each against the shipped path (tests/test_gpu_flow.py::test_every_kernel_variant_in_the_library_agrees...) and DESIGN.md section 6 quotes
// its measurement.  fc_debug_set / _get / _name / _reset (ops_api.cpp; bench.py --knob K=V, profiles/) reach them by key.
// One X(key, field, shipped default, accepted values as an expression in v, description) line per knob.  The accepted set is exactly the
// set of values the reading code distinguishes: fc_debug_set refuses any other (FC_ERR_UNSUPPORTED) and leaves the setting as it was; keys
// not listed (3, 15, 17, 19, 21, 27, 29, 30, ...: variants that lost an A/B and were removed) are FC_ERR_INVALID.
// The members are plain ints read on the host launch path: set them between calls, not while another thread launches.
#pragma once

#define FC_KNOBS(X) \
    X(0, gemm_variant, 5, v == 2 || v == 3 || v == 5, "GEMM main loop: 5 = split-fp16 (shipped), 3 = split-bf16 (the range fallback), 2 = fp32-input MFMA (the reference loop)") \
    X(2, gemm_colgroup, 10, v >= 0, "column-group size of the row-band tile order for weight matrices that do not fit L2 (0 = plain order)") \
    X(5, attn_fp16, 1, v == 0 || v == 1, "attention on the split-fp16 kernel inside a guard scope (shipped); 0 keeps the fp32-input MFMA kernel") \
    X(7, fused_spline, 1, v == 0 || v == 1, "1 = the spline coupling is evaluated in the epilogue of the GEMM that makes its parameters (shipped; the limb chain needs it), 0 = the parameter matrix goes through HBM to launch_spline") \
    X(8, premlp_fused, 2, v == 0 || v == 2, "pre-attention chain: 2 = the row-resident kernel (premlp.hip, activations in registers; shipped: 190 us against ~250 us for the five launches it replaces, -1.4 ... -2 % per C2 step; the removed LDS-tile kernel, value 1, took 263 us: one 64-row workgroup per CU re-streams every layer's weights from L2, 16 % MFMA busy), 0 = separate GEMM launches + the LayerNorm -> q fold") \
    X(9, limb_chain, 1, v == 0 || v == 1, "1 = the layer before a coupling's parameter GEMM (and the stacked K|V projection) writes its output as the limb image the consumer copies (shipped), 0 = fp32 panels, re-split per column tile") \
    X(10, lnq_fold, 1, v == 0 || v == 1, "1 = out_layer, LayerNorm and the q projection of a pre-attention chain as ONE GEMM (EPI_LNQ) + a finalize pass (shipped), 0 = three launches") \
    X(11, train_wgrad16, 1, v == 0 || v == 1, "training: weight gradients on the split-fp16 loop inside a guard scope (shipped)") \
    X(12, train_attn16, 1, v == 0 || v == 1, "training: attention backward on the split-fp16 loop inside a guard scope (head dim 64; shipped)") \
    X(13, spline_kernel, 5, v == 2 || v == 4 || v == 5, "fused spline GEMM: 5 = 256 x 256 one-accumulator tile on 16x16x32 MFMAs (spline_wide.hip, shipped; K = 8 bins, limb-chained input; other launches fall to 4), 4 = persistent transposed LDS-DMA loop, splines evaluated from the accumulator registers (VAR 11; K = 8 bins), 2 = LDS-DMA loop on the 128x128 four-wave tile with the LDS parameter tile (VAR 9; 4 and 16 bins always); bit-identical results") \
    X(14, spline_ablate, 0, v >= 0 && v <= 5, "diagnostics, results invalid: 1 = fused spline epilogue without the spline evaluation, 2 = main loop only, 3 = no parameter-tile write, 4 = no x2 store, 5 = stop behind the tile write (3..5 exist on the LDS-tile epilogue only and keep the wide kernel off)") \
    X(16, limb_chain_all, 1, v == 0 || v == 1, "1 = every hidden activation of the coupling MLP exists only as a limb image (A16 / residual16 / C16; shipped), 0 = also as fp32") \
    X(20, stamps, 0, v >= 0 && v <= 4, "diagnostic: in-kernel phase stamps (read back with fc_debug_gemm_stamps) of 1 = the LDS-DMA fused spline launches, 2 = the limb-chained Linear launches, 3 = the row-resident pre-attention kernel, 4 = the row-resident coupling MLP") \
    X(22, small_tiles, 1, v == 0 || v == 1, "1 = limb-chained Linear launches with at most 256 tiles of 128x128 run on 64x64 tiles (shipped)") \
    X(23, mlp_rows, 1, v >= 0 && v <= 2, "1 = row-resident coupling MLP chain (mlprows.hip) where it fills the chip (shipped), 2 = at any size (tests), 0 = one GEMM launch per layer") \
    X(24, knn_mfma, 1, v >= 0 && v <= 2, "k-NN: 1 = Gram tiles on the matrix cores + sorted register lists where the launch fills the chip (shipped), 2 = always (tests), 0 = the lane-per-candidate kernel") \
    X(26, premlp_lu, 1, v == 0 || v == 1, "1 = the previous layer's folded ActNorm + LU runs as a pre-layer of the row-resident pre-attention kernel (shipped), 0 = as its own GEMM launch") \
    X(28, spline_wide_colgroup, -1, v >= -1, "wide fused spline kernel: column-group size of the tile order in 256-column tiles (-1 = shipped: 5)") \
    X(31, train_wide, 1, v == 0 || v == 1, "1 = training Linear layers with at least 1024 outputs (the spline parameter layer) on the 256 x 256 one-accumulator loop (shipped), 0 = on the fp32-A 128 x 128 loop") \
    X(32, knn_warm, 1, v == 0 || v == 1, "1 = a DGCNN level's k-NN search starts from the previous level's neighbour sets where the caller hands them over (shipped; exact either way), 0 = never") \
    X(33, kv_fold, 1, v == 0 || v == 1, "read by fc_flow_create: 1 = to_kv folded into the q projections and the consumers' in_layers where the gate allows it, keys = values = the context panel (shipped), 0 = the stacked K|V projection") \
    X(34, spline_fold, 1, v == 0 || v == 1, "read by fc_flow_create: 1 = the wide spline kernel's image holds the 22 informative parameters per dim on 112-column wave tiles (shipped), 0 = all 25 on 128-column tiles")

namespace fc {

struct Knobs {
#define FC_KNOB_FIELD(key, field, def, accept, doc) int field = def;
    FC_KNOBS(FC_KNOB_FIELD)
#undef FC_KNOB_FIELD
};
extern Knobs g_knobs;      // defined in ops_api.cpp

}  // namespace fc
