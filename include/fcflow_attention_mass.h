/* libfcflow: attention mass per context point -- an addition to fcflow.h in a header of its own.  FC_ABI_VERSION stays 10, nothing
 * declared in fcflow.h changes; the conventions are those of fcflow.h (no allocation inside a call, an explicit stream, an int
 * status with the cause in the last-error text).
 *
 *   mass[b, j] = sum_p g[b, p] * softmax_j( q[b, p, :] . k[b, j, :] )          p < N, j < M
 *
 * the weighted column sums of the softmax rows that the attention-weights entry points of fcflow.h export: how much of the target
 * cloud's attention (g = ones), of its change score (g = the change) or of a subset (g = a 0/1 mask) lands on every context point.
 * The [B, N, M] map is never formed: the probabilities are reduced on the chip (csrc/attention_mass.hip).
 * The result is the same bytes on every run: no float atomics, all partial sums are added in a fixed order. */
#ifndef FCFLOW_ATTENTION_MASS_H
#define FCFLOW_ATTENTION_MASS_H

#include "fcflow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of the call below: the forward's workspace (what the flow's own workspace query returns, which does not change)
 * plus the slab region behind it: 256-byte alignment + 4 * B * ceil(N / 128) * M bytes, shared by all requested layers. */
int fc_flow_attention_mass_workspace_bytes(const fc_flow* flow, int32_t B, int32_t N, int32_t M, size_t* bytes);

/* The forward of the log-prob entry that additionally writes, for each of n_layers requested attentions, the attention mass of
 * the M context points: out[i] is a device buffer [B, M] fp32.  Layer ids and refusals are those of the attention-weights entry:
 * -1 = the augmenter's attention, 0 .. n_flow_layers-1 = the pre-conditioner of that flow layer; FC_ERR_INVALID before anything
 * is launched for a flow layer without attention, -1 on a flow whose first transform is IdentityTransform, an id out of range.
 * row_weight: device [B, N] fp32 or NULL (= ones), the same weights at every layer.  logprob [B, N] may be NULL.  A workspace
 * smaller than the query above asks for is FC_ERR_WORKSPACE.  A pass repeated on the bf16 limbs rewrites slabs and outputs. */
int fc_flow_attention_mass_f32(fc_flow* flow, const float* x, const float* ctx, const float* extra, const float* const* eps,
                               int32_t n_eps, const int32_t* layers, int32_t n_layers, const float* row_weight, float* const* out,
                               float* logprob, int32_t B, int32_t N, int32_t M, void* workspace, size_t workspace_bytes, void* stream);

/* Scratch of the operator below: 4 * B * ceil(N / 128) * M bytes (one fp32 row of M partial sums per 128 queries of a scene). */
size_t fc_op_attention_mass_scratch_bytes(int32_t B, int32_t N, int32_t M);

/* out[B,M] = sum over p of row_weight[b,p] * softmax(q k^T * scale)[b,p,:] with q [B,N,D], k [B,M,D], D in {32, 64, 128, 256}:
 * the kernels of the flow entry above alone.  row_weight [B,N] or NULL (= ones).  scratch: device memory, 16-byte aligned, of
 * at least the size above (FC_ERR_WORKSPACE when smaller).  Synchronises the stream like the other single-operator calls. */
int fc_op_attention_mass_f32(const float* q, const float* k, const float* row_weight, float* out, int32_t B, int32_t N, int32_t M,
                             int32_t D, float scale, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FCFLOW_ATTENTION_MASS_H */
