/* libfcflow: the DGCNN embedder with per-scene point counts -- an addition to fcflow.h in a header of its own.  The ABI version stays 10,
 * nothing declared in fcflow.h, fcflow_attention_mass.h, fcflow_context_counts.h or fcflow_sparse_stage.h changes; the conventions are
 * those of fcflow.h (an explicit stream, an int status with the cause in the last-error text).
 *
 * fc_dgcnn_embed_f32 (fcflow.h) takes one M for the whole batch.  The entries below take the same padded batch plus counts, a DEVICE array
 * [B] of int32: scene b is its first counts[b] rows, and gets bit for bit what it gets when passed alone as pts[b:b+1, :counts[b]].  In
 * eval mode a DGCNN row depends on its scene through the k-NN search, the gather-max behind it and the global pool only, and those three
 * take the count; everything else runs row-wise on the padded batch.  Rows counts[b] .. M-1 of a scene are padding:
 * what they hold (zeros, NaN, 1e30) changes neither the result nor whether the pass is repeated on the bf16 limbs.
 * count_min / count_max are HOST integers the caller vouches for, k <= count_min <= min_b counts[b], max_b counts[b] <= count_max <= M:
 * kernels and grids are chosen by them without a read-back, and the kernels clamp every count into [count_min, count_max], so that a
 * device array that disagrees with them reaches neither an out-of-range row nor a kernel that was not launched (the Python binding
 * checks the array first).  Refused with FC_ERR_INVALID: a NULL counts (use the entries of fcflow.h) and bounds that are not
 * k <= count_min <= count_max <= M. */
#ifndef FCFLOW_EMBED_COUNTS_H
#define FCFLOW_EMBED_COUNTS_H

#include "fcflow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fc_dgcnn_embed_f32 with counts behind pts.  out: [B, M, E] for a per-point embedder, rows >= counts[b] written as 0.0f (no
 * initialisation needed); [B, E] for a global one, pooled over the scene's own rows.  Workspace: fc_dgcnn_workspace_bytes(emb, B, M).
 * No allocation, no synchronisation. */
int fc_dgcnn_embed_counts_f32(fc_dgcnn* emb, const float* pts, const int32_t* counts, int32_t count_min, int32_t count_max, float* out,
                              int32_t B, int32_t M, void* workspace, size_t workspace_bytes, void* stream);

/* fc_op_knn_f32 / fc_op_knn_warm_f32 with counts: f [B, M, C], idx [B, M, k]; idx[b, :counts[b]] are the sets of the search over
 * f[b, :counts[b]] alone, by the kernel that search takes alone (a batch on both sides of the kernel threshold costs two launches);
 * rows >= counts[b] of idx are written by nobody.  idx_warm_or_null: warm sets [B, M, k] (may equal idx) or NULL for a cold search.
 * Synchronises the stream, like its namesakes. */
int fc_op_knn_counts_f32(const float* f, const int32_t* idx_warm_or_null, const int32_t* counts, int32_t count_min, int32_t count_max,
                         int32_t* idx, int32_t B, int32_t M, int32_t C, int32_t k, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FCFLOW_EMBED_COUNTS_H */
