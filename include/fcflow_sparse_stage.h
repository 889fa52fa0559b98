/* libfcflow: scene staging of voxels with sparse context -- an addition to fcflow.h in a header of its own.  The ABI version stays 10,
 * nothing declared in fcflow.h, fcflow_attention_mass.h or fcflow_context_counts.h changes; the conventions are those of fcflow.h (no
 * allocation, an explicit stream, no synchronisation, an int status with the cause in the last-error text).
 *
 * fc_stage_fps_ragged_f32 (fcflow.h) takes m picks of every listed voxel and refuses a voxel with fewer than m rows.  The entries below
 * stage voxels whose context box holds FEWER rows than the sample count: such a voxel keeps all its rows, its slots behind them are
 * padding, and a device array of int32 says how many slots are real -- the `ctx_counts` the entries of fcflow_context_counts.h take.
 * The library cannot validate a device array without a synchronisation: row numbers are clamped into their cloud on load and counts
 * into [1, M].  Outputs need no initialisation: every element is written, padding included. */
#ifndef FCFLOW_SPARSE_STAGE_H
#define FCFLOW_SPARSE_STAGE_H

#include "fcflow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fc_stage_fps_ragged_f32 with a sample count per voxel: listed voxel v with n_v rows takes m_v = min(n_v, m) picks, the same loop,
 * reduction order, tie rule and distance arithmetic.  idx [n_voxels, m]: idx[v, :m_v] are the first m_v picks (cloud row numbers),
 * idx[v, m_v:] the literal -1; sample_counts [n_voxels] int32: m_v.  A voxel without rows writes count 0 and a row of -1.  max_rows
 * bounds the listed voxels' sizes as there, and m may exceed it (every listed voxel sparse).  dist_scratch as there: a float per entry
 * of `rows` when max_rows > 24576, else NULL. */
int fc_stage_fps_ragged_counts_f32(const float* cloud, int32_t ld, int32_t C, int64_t P, const int64_t* offsets, const int32_t* rows,
                                   const int32_t* voxel_ids, int32_t n_voxels, int32_t max_rows, int32_t m, int64_t* idx, int32_t* sample_counts,
                                   float* dist_scratch, void* stream);

/* Gather and joint unit-sphere normalisation of n_pairs voxel pairs straight through their index lists, one workgroup per pair:
 * pair k = (cloud_0[index_0[k, :c_k]], cloud_1[index_1[k]]) with c_k = counts_0[k] clamped into [1, M]; cloud_0 [P0, ld], cloud_1 [P1, ld]
 * contiguous, ld = 3..8 columns (xyz first), index_0 [n_pairs, M] / index_1 [n_pairs, N] int64 as the FPS entries write them (the -1
 * behind c_k is never read).  out_0 [n_pairs, M, ld], out_1 [n_pairs, N, ld], inverse [n_pairs, 4] = furthest distance, mean xyz:
 * bit for bit what fc_stage_co_unit_sphere_f32 gives for the pair; rows >= c_k of out_0[k] are written as 0.0f in every column. */
int fc_stage_pairs_counts_f32(const float* cloud_0, int64_t P0, const float* cloud_1, int64_t P1, int32_t ld, const int64_t* index_0,
                              const int64_t* index_1, const int32_t* counts_0, int32_t n_pairs, int32_t M, int32_t N, float* out_0, float* out_1,
                              float* inverse, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FCFLOW_SPARSE_STAGE_H */
