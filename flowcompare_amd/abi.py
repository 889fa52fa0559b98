"""The C ABI of libfcflow.so as ctypes sees it: one line per entry point, (return kind, parameter kinds).

ENTRIES follows include/fcflow.h in the header's order; DEBUG_ENTRIES are the fc_debug_* diagnostics that csrc/ops_api.cpp defines
without a declaration in the header.  tests/test_host.py compares both tables with the C sources.  EXTRA_ENTRIES are the entry points
declared in headers of their own behind fcflow.h (include/fcflow_attention_mass.h; tests/test_attention_mass_host.py), COUNTS_ENTRIES
those of include/fcflow_context_counts.h (tests/test_context_counts_host.py), SPARSE_STAGE_ENTRIES those of include/fcflow_sparse_stage.h
(tests/test_sparse_stage_host.py), EMBED_COUNTS_ENTRIES those of include/fcflow_embed_counts.h (tests/test_embed_counts_host.py), SPARSE_TARGET_ENTRIES those of
include/fcflow_sparse_target.h (tests/test_sparse_target_host.py), PACONV_COUNTS_ENTRIES those of include/fcflow_paconv_counts.h
(tests/test_paconv_counts_host.py).

Parameter kinds:  P  any pointer (handles, struct pointers, const char*, the stream)     i  int32_t / int     l  int64_t
                  f  float     z  size_t
Return kinds:     status  an FC_* code: bind() gives the entry an errcheck that raises on a non-zero one
                  int / int64 / size_t / str (const char*) / void  a value, handed back as it is
"""
import ctypes

PARAM_KINDS = {"P": ctypes.c_void_p, "i": ctypes.c_int32, "l": ctypes.c_int64, "f": ctypes.c_float, "z": ctypes.c_size_t}
RETURN_KINDS = {"status": ctypes.c_int, "int": ctypes.c_int, "int64": ctypes.c_int64, "size_t": ctypes.c_size_t, "str": ctypes.c_char_p,
                "void": None}

ENTRIES = {
    "fc_abi_version":                        ("int", ""),
    "fc_last_error":                         ("str", ""),
    "fc_flow_create":                        ("status", "PPiP"),
    "fc_flow_destroy":                       ("void", "P"),
    "fc_flow_workspace_bytes":               ("status", "PiiiP"),
    "fc_flow_noise_count":                   ("int", "P"),
    "fc_flow_noise_width":                   ("int", "Pi"),
    "fc_flow_logprob_f32":                   ("status", "PPPPPiPPiiiPzP"),
    "fc_flow_attention_weights_f32":         ("status", "PPPPPiPiPiiPPiiiPzP"),
    "fc_flow_inverse_f32":                   ("status", "PPPPPiPiiiPzP"),
    "fc_dgcnn_create":                       ("status", "iiPiP"),
    "fc_dgcnn_destroy":                      ("void", "P"),
    "fc_dgcnn_out_dim":                      ("int", "P"),
    "fc_dgcnn_workspace_bytes":              ("status", "PiiP"),
    "fc_dgcnn_embed_f32":                    ("status", "PPPiiPzP"),
    "fc_paconv_create":                      ("status", "PiP"),
    "fc_paconv_destroy":                     ("void", "P"),
    "fc_paconv_out_dim":                     ("int", "P"),
    "fc_paconv_workspace_bytes":             ("status", "PiiP"),
    "fc_paconv_embed_f32":                   ("status", "PPPiiPzP"),
    "fc_op_fps_f32":                         ("status", "PPiiiP"),
    "fc_stage_fps_f32":                      ("status", "PiiPiiiP"),
    "fc_stage_co_unit_sphere_f32":           ("status", "PiPiiPPPiP"),
    "fc_stage_voxel_ws_bytes":               ("size_t", "li"),
    "fc_stage_voxel_count_f32":              ("status", "PilPifffPPzP"),
    "fc_stage_voxel_select_f32":             ("status", "PilPifffPPlPzP"),
    "fc_stage_fps_ragged_f32":               ("status", "PiilPPPiiiPPP"),
    "fc_clamp_infs_f32":                     ("status", "PlP"),
    "fc_change_map_f32":                     ("status", "PiPiPiffiPP"),
    "fc_range_check_defer":                  ("status", "i"),
    "fc_range_check_resolve":                ("status", "P"),
    "fc_range_check_pending":                ("int", ""),
    "fc_profile_enable":                     ("status", "i"),
    "fc_profile_reset":                      ("status", ""),
    "fc_profile_filter":                     ("status", "P"),
    "fc_profile_stride":                     ("status", "i"),
    "fc_profile_report":                     ("status", "Pz"),
    "fc_op_linear_f32":                      ("status", "PPPPPiiiiP"),
    "fc_op_mlp_hidden_f32":                  ("status", "PiPiPPiPiiiP"),
    "fc_op_attention_f32":                   ("status", "PPPPiiiifP"),
    "fc_op_attention_weights_f32":           ("status", "PPPPiiiiiifP"),
    "fc_op_knn_f32":                         ("status", "PPiiiiP"),
    "fc_op_knn_warm_f32":                    ("status", "PPPiiiiP"),
    "fc_op_expm_action_f32":                 ("status", "PiPiPPiPPiiiP"),
    "fc_op_rqspline_f32":                    ("status", "PPPPliiP"),
    "fc_train_linear_pack_bytes":            ("size_t", "iPi"),
    "fc_train_linear_pack_f32":              ("status", "PPiPiPzPP"),
    "fc_train_linear_fwd_f32":               ("status", "PiPiPPiPiPiPP"),
    "fc_train_linear_act_fwd_f32":           ("status", "PiPiPPiPiPPiiPP"),
    "fc_train_linear_dgrad_f32":             ("status", "PiPiPiiPiPPP"),
    "fc_train_linear_dgrad_act_f32":         ("status", "PiPiPiiPiPPiPPP"),
    "fc_train_linear_wgrad_ws_bytes":        ("size_t", "iPii"),
    "fc_train_linear_wgrad_f32":             ("status", "iPiPiPPiPPiPzPP"),
    "fc_train_act_fwd_f32":                  ("status", "PPiiiP"),
    "fc_train_act_bwd_f32":                  ("status", "PPPiiiiP"),
    "fc_train_attention_ws_bytes":           ("size_t", "iiii"),
    "fc_train_attention_fwd_f32":            ("status", "PiPiPiPiiiiifPzPPPP"),
    "fc_train_attention_bwd_f32":            ("status", "PiPiPiPiPiPiPiPiPiiiiifPP"),
    "fc_train_rqspline_fwd_f32":             ("status", "PiPiPiPiiiP"),
    "fc_train_rqspline_bwd_f32":             ("status", "PiPiPiPPiPiiiiPP"),
    "fc_train_layernorm_fwd_f32":            ("status", "PiPPPiPiifP"),
    "fc_train_layernorm_bwd_f32":            ("status", "PiPPiPPiPiiiiP"),
    "fc_train_affine_fwd_f32":               ("status", "PiPiPiPiiiP"),
    "fc_train_affine_bwd_f32":               ("status", "PiPiPiPPiPiiiiP"),
    "fc_train_gauss_fwd_f32":                ("status", "PiPPiPiifP"),
    "fc_train_gauss_bwd_f32":                ("status", "PiPPiPPiiifP"),
    "fc_train_normlp_fwd_f32":               ("status", "PiPiPiifP"),
    "fc_train_normlp_bwd_f32":               ("status", "PiPiPPiPiiifP"),
    "fc_train_expm_fwd_f32":                 ("status", "PiPiPPiPiiPP"),
    "fc_train_expm_bwd_f32":                 ("status", "PiPiPPiPPiPiPiiP"),
    "fc_train_expm_wide_bwd_f32":            ("status", "PiPiPPiPPiPiPiiPP"),
    "fc_train_base_fwd_f32":                 ("status", "PiPiiP"),
    "fc_train_base_bwd_f32":                 ("status", "PiPPiiiP"),
    "fc_train_colsum_ws_bytes":              ("size_t", "ii"),
    "fc_train_colsum_f32":                   ("status", "PiiiPiPzP"),
    "fc_train_edge_ws_bytes":                ("size_t", "ii"),
    "fc_train_edge_stats_f32":               ("status", "PiPiPiiifPPzP"),
    "fc_train_edge_fwd_f32":                 ("status", "PiPiPiiiPPPfPiPP"),
    "fc_train_edge_bwd_prep_f32":            ("status", "PiPiPiiiPPPfPPiPPiiP"),
    "fc_train_pool_fwd_f32":                 ("status", "PiiiiPiPP"),
    "fc_train_pool_bwd_f32":                 ("status", "PiPiiiPiP"),
    "fc_train_edge_bwd_gather_f32":          ("status", "PiPiPiiiPPPPiPPPPPiP"),
    "fc_train_edge_bwd_scatter_f32":         ("status", "PiPiPiiiPPPPiPPPiPiP"),
    "fc_op_paconv_knn_f32":                  ("status", "PPPiiiiP"),
    "fc_train_paconv_group_f32":             ("status", "PPiiPPPiPiiiiP"),
    "fc_train_softmax_fwd_f32":              ("status", "PiiiPiP"),
    "fc_train_softmax_bwd_f32":              ("status", "PiPiiiiPiP"),
    "fc_train_assign_fwd_f32":               ("status", "PiPiiiiiPiP"),
    "fc_train_assign_bwd_f32":               ("status", "PiPiPiiiiiPiPiP"),
    "fc_train_centerdiff_fwd_f32":           ("status", "PiiiiPiP"),
    "fc_train_centerdiff_bwd_f32":           ("status", "PiiiiPiP"),
    "fc_train_rows_gather_bwd_f32":          ("status", "PiiiPPPiiiPiP"),
    "fc_train_three_nn_f32":                 ("status", "PPiiiPPP"),
    "fc_train_interp_fwd_f32":               ("status", "PiiPPiiPiP"),
    "fc_train_sqnorm_ws_bytes":              ("size_t", "l"),
    "fc_train_sqnorm_f32":                   ("status", "PlPiPzP"),
    "fc_train_adam_f32":                     ("status", "PPPPiPPPPfffffiP"),
    "fc_stage_dense_blocks_f32":             ("status", "PiilPPPiPPiPPPP"),
    "fc_change_map_ragged_f32":              ("status", "PPPiPiffiPP"),
}

# Entry points declared in a header of their own behind fcflow.h: include/fcflow_attention_mass.h, in that header's order
# (tests/test_attention_mass_host.py compares).  Status entries raise like those of ENTRIES.
EXTRA_ENTRIES = {
    "fc_flow_attention_mass_workspace_bytes": ("status", "PiiiP"),
    "fc_flow_attention_mass_f32":            ("status", "PPPPPiPiPPPiiiPzP"),
    "fc_op_attention_mass_scratch_bytes":    ("size_t", "iii"),
    "fc_op_attention_mass_f32":              ("status", "PPPPiiiifPzP"),
}

# Per-scene context point counts: include/fcflow_context_counts.h, in that header's order (tests/test_context_counts_host.py compares).
# The namesakes of ENTRIES / EXTRA_ENTRIES with `ctx_counts` (device int32 [B]) directly behind ctx; status entries raise like those of ENTRIES.
COUNTS_ENTRIES = {
    "fc_flow_logprob_counts_f32":            ("status", "PPPPPPiPPiiiPzP"),
    "fc_flow_attention_weights_counts_f32":  ("status", "PPPPPPiPiPiiPPiiiPzP"),
    "fc_flow_attention_mass_counts_f32":     ("status", "PPPPPPiPiPPPiiiPzP"),
    "fc_op_attention_counts_f32":            ("status", "PPPPPiiiifP"),
    "fc_op_attention_ctx_counts_f32":        ("status", "PPPPiiiifP"),
}

# Scene staging of voxels with sparse context: include/fcflow_sparse_stage.h, in that header's order (tests/test_sparse_stage_host.py compares).
SPARSE_STAGE_ENTRIES = {
    "fc_stage_fps_ragged_counts_f32":        ("status", "PiilPPPiiiPPPP"),
    "fc_stage_pairs_counts_f32":             ("status", "PlPliPPPiiiPPPP"),
}

# The DGCNN embedder with per-scene point counts: include/fcflow_embed_counts.h, in that header's order (tests/test_embed_counts_host.py compares).
EMBED_COUNTS_ENTRIES = {
    "fc_dgcnn_embed_counts_f32":             ("status", "PPPiiPiiPzP"),
    "fc_op_knn_counts_f32":                  ("status", "PPPiiPiiiiP"),
}

# Voxels with few target points: include/fcflow_sparse_target.h, in that header's order (tests/test_sparse_target_host.py compares).
SPARSE_TARGET_ENTRIES = {
    "fc_stage_pairs_counts2_f32":            ("status", "PlPliPPPPiiiPPPP"),
    "fc_change_map_counts_f32":              ("status", "PiPPiPPiffiPP"),
    "fc_change_map_ragged_counts_f32":       ("status", "PPPiPPiffiPP"),
}

# The PAConv embedder with per-scene point counts: include/fcflow_paconv_counts.h, in that header's order (tests/test_paconv_counts_host.py compares).
PACONV_COUNTS_ENTRIES = {
    "fc_paconv_embed_counts_f32":            ("status", "PPPiiPiiPzP"),
    "fc_op_fps_counts_f32":                  ("status", "PPiiPiiiP"),
    "fc_op_paconv_knn_counts_f32":           ("status", "PPPPPiiiiP"),
}

# Diagnostics and test hooks: they hand back their raw code and never raise (a caller compares fc_debug_set(...) with 0).
DEBUG_ENTRIES = {
    "fc_debug_set":                          ("int", "ii"),
    "fc_debug_get":                          ("int", "iP"),
    "fc_debug_reset":                        ("int", ""),
    "fc_debug_name":                         ("str", "i"),
    "fc_debug_one_acc_gemm_f32":             ("int", "PPPfPiiiP"),
    "fc_debug_spline_col":                   ("int", "iii"),
    "fc_debug_spline_tile_pos":              ("int", "ii"),
    "fc_debug_kv_fold_gate":                 ("int", "iiii"),
    "fc_debug_gemm_stamps":                  ("int64", "Pl"),
    "fc_debug_flow_trace":                   ("int", "Pl"),
    "fc_debug_expm_info":                    ("int", "Pl"),
    "fc_debug_fp16_fallbacks":               ("int64", ""),
    "fc_debug_attention_ctx_f32":            ("int", "PPPiiiifP"),
    "fc_debug_premlp_q_f32":                 ("int", "PiiPiPiPPiiiP"),
}


def bind(L, status_errcheck):
    """Sets argtypes and restype of every table entry the loaded library has; a status entry of ENTRIES also gets `status_errcheck`.
    A symbol the library lacks is skipped (an FCFLOW_LIB build of this ABI version that predates an entry still loads) and fails
    with AttributeError at the call."""
    for table in (ENTRIES, EXTRA_ENTRIES, COUNTS_ENTRIES, SPARSE_STAGE_ENTRIES, EMBED_COUNTS_ENTRIES, SPARSE_TARGET_ENTRIES, PACONV_COUNTS_ENTRIES,
                  DEBUG_ENTRIES):
        for name, (ret, params) in table.items():
            fn = getattr(L, name, None)
            if fn is None:
                continue
            fn.argtypes = [PARAM_KINDS[k] for k in params]
            fn.restype = RETURN_KINDS[ret]
            if ret == "status" and table is not DEBUG_ENTRIES:
                fn.errcheck = status_errcheck
