/* libfcflow: scene change maps of voxels with few TARGET points -- an addition to fcflow.h in a header of its own.  The ABI version stays 10,
 * nothing declared in fcflow.h, fcflow_attention_mass.h, fcflow_context_counts.h, fcflow_sparse_stage.h or fcflow_embed_counts.h changes; the
 * conventions are those of the namesakes: an explicit stream, an int status with the cause in the last-error text, no allocation and no
 * synchronisation beyond what the namesake does (the change-map entries read their status word back, as fc_change_map_f32 does).
 *
 * fcflow_sparse_stage.h gave the CONTEXT side of a staged voxel a count of its own.  The entries below do the same for the target side
 * (DESIGN.md section 11j): a voxel whose final box holds fewer rows than the sample count keeps all of them, the slots behind them are
 * padding, and a device array of int32 says how many slots are real.  The library cannot validate a device array without a
 * synchronisation: row numbers are clamped into their cloud on load and counts into [1, row length].  Pad slots of an input are never
 * read and never written; every element of an output is written, padding included. */
#ifndef FCFLOW_SPARSE_TARGET_H
#define FCFLOW_SPARSE_TARGET_H

#include "fcflow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fc_stage_pairs_counts_f32 (fcflow_sparse_stage.h) with a count on both sides, one workgroup per pair: pair k =
 * (cloud_0[index_0[k, :c_k]], cloud_1[index_1[k, :n_k]]) with c_k = counts_0[k] clamped into [1, M] (counts_0 NULL: c_k = M) and
 * n_k = counts_1[k] clamped into [1, N]; the -1 behind a count is never read.  out_0 [n_pairs, M, ld], out_1 [n_pairs, N, ld], inverse
 * [n_pairs, 4] = furthest distance, mean xyz: bit for bit what fc_stage_co_unit_sphere_f32 gives for the truncated pair; rows >= c_k of
 * out_0[k] and rows >= n_k of out_1[k] are written as 0.0f in every column.  With every n_k = N the bytes of fc_stage_pairs_counts_f32. */
int fc_stage_pairs_counts2_f32(const float* cloud_0, int64_t P0, const float* cloud_1, int64_t P1, int32_t ld, const int64_t* index_0,
                               const int64_t* index_1, const int32_t* counts_0, const int32_t* counts_1, int32_t n_pairs, int32_t M, int32_t N,
                               float* out_0, float* out_1, float* inverse, void* stream);

/* fc_change_map_f32 with a length per row on both sides: scene b owns the first n1_b = counts_1[b] (clamped into [1, N]) values of
 * lp10[b] and the first n0_b = counts_0[b] (clamped into [1, N0]; counts_0 NULL: N0) values of lp00[b], and gets fc_change_map_f32's rules,
 * arithmetic and summation order on those.  The inf statistics of each tensor (an inf seen, the smallest non-inf value) are taken over
 * real slots only.  Slots >= n1_b of out[b] are written as NaN (not evaluated).  Without a hard cutoff a baseline row needs two values (the
 * unbiased std divides by n0_b - 1): a shorter one raises bit 2 of *invalid (value 4), and its scene's output row is all NaN; bit 0 (value
 * 1) is fc_change_map_f32's flag.  With all counts full the bytes of fc_change_map_f32.  Synchronises the stream. */
int fc_change_map_counts_f32(float* lp10, int32_t N, const int32_t* counts_1, float* lp00, int32_t N0, const int32_t* counts_0, float* out, int32_t B,
                             float multiple, float hard_cutoff, int32_t use_cutoff, int32_t* invalid, void* stream);

/* fc_change_map_ragged_f32 with a baseline length per voxel: counts_0 [B] (NULL: N0 for every voxel) as above, lp10 / out flat as there.
 * *invalid as for fc_change_map_counts_f32, except that a voxel without rows contributes nothing and its baseline length is not checked;
 * with counts_0 NULL or full the bytes of fc_change_map_ragged_f32.  Synchronises the stream. */
int fc_change_map_ragged_counts_f32(float* lp10, const int64_t* offsets, float* lp00, int32_t N0, const int32_t* counts_0, float* out, int32_t B,
                                    float multiple, float hard_cutoff, int32_t use_cutoff, int32_t* invalid, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FCFLOW_SPARSE_TARGET_H */
