/* libfcflow: the PAConv embedder with per-scene point counts -- an addition to fcflow.h in a header of its own.  The ABI version stays 10,
 * nothing declared in fcflow.h or in the other headers behind it changes; the conventions are those of fcflow.h (an explicit stream, an int
 * status with the cause in the last-error text) and of fcflow_embed_counts.h (counts: a DEVICE array [B] of int32; count_min / count_max:
 * HOST bounds the caller vouches for, by which kernels and grids are chosen without a read-back; the kernels clamp every count into them,
 * so that a device array that disagrees reaches neither an out-of-range row nor a kernel that was not launched; the one launch that
 * zeroes the pad rows of the level-0 panels clamps into [1, M] instead, as in the DGCNN engine: under a count below count_min it zeroes rows
 * that the kernels then read as points at the origin -- nothing out of range, but the result is that of no valid input).
 *
 * fc_paconv_embed_f32 (fcflow.h) takes one M for the whole batch.  The entry below takes the same padded batch plus counts: scene b is its
 * first counts[b] rows and gets bit for bit what it gets when passed alone as pts[b:b+1, :counts[b]].  In eval mode a PAConv row depends on
 * its scene through five kernels only -- farthest point sampling, the xyz gather, the 32-NN, the grouping and the 3-NN interpolation --
 * and those take the count; everything else runs row-wise on the padded batch.  Level l of scene b keeps its place
 * b * (M >> 2l) in the workspace and uses its first counts[b] >> 2l rows, so fc_paconv_workspace_bytes(emb, B, M) is the workspace of both
 * calls.  Rows counts[b] .. M-1 of a scene are padding: what they hold (zeros, NaN, 1e30) changes neither the result nor whether the pass is
 * repeated on the bf16 limbs. */
#ifndef FCFLOW_PACONV_COUNTS_H
#define FCFLOW_PACONV_COUNTS_H

#include "fcflow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fc_paconv_embed_f32 with counts behind pts.  out: [B, M, E], rows >= counts[b] written as 0.0f (no initialisation needed).  Refused with
 * FC_ERR_INVALID before any launch: a NULL handle, workspace, pts, counts or out, and bounds that are not
 * 256 <= count_min <= count_max <= M (the embedder's four 4x down-samplings need 256 points of every scene).  No allocation, no
 * synchronisation. */
int fc_paconv_embed_counts_f32(fc_paconv* emb, const float* pts, const int32_t* counts, int32_t count_min, int32_t count_max, float* out,
                               int32_t B, int32_t M, void* workspace, size_t workspace_bytes, void* stream);

/* fc_op_fps_f32 with counts, exactly as the engine launches it: xyz [B, n, 3], idx [B, m] with m == n >> 2.  Scene b samples
 * m_b = counts[b] >> 2 of its first counts[b] rows with the virtual thread count it uses alone; idx[b, :m_b] are the picks of fc_op_fps_f32
 * on xyz[b:b+1, :counts[b]], idx[b, m_b:] is written as -1.  Whether the coordinates live in LDS or are read from memory is chosen by n
 * (above 8192: memory, the scratch is allocated stream-ordered as in fc_op_fps_f32); both do the same arithmetic with the same ties.
 * Bounds: 4 <= count_min <= count_max <= n. */
int fc_op_fps_counts_f32(const float* xyz, const int32_t* counts, int32_t count_min, int32_t count_max, int32_t* idx, int32_t B, int32_t n,
                         int32_t m, void* stream);

/* fc_op_paconv_knn_f32 with counts: xyz [B, n, 4], qxyz [B, m, 4], out [B, m, k] (k <= 32).  Scene b's candidates are its first
 * counts_n[b] rows of xyz (clamped into [1, n]) and its queries its first counts_m[b] rows of qxyz (clamped into [0, m]);
 * out[b, :counts_m[b]] is what fc_op_paconv_knn_f32 gives on the scene alone (counts_n[b] < k: the tail keeps index 0), rows behind it are
 * written as zeros.  The per-lane list length is chosen by n; any sufficient length gives the same result. */
int fc_op_paconv_knn_counts_f32(const float* xyz, const float* qxyz, const int32_t* counts_n, const int32_t* counts_m, int32_t* out,
                                int32_t B, int32_t n, int32_t m, int32_t k, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FCFLOW_PACONV_COUNTS_H */
