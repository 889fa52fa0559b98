/* libfcflow: per-scene context point counts -- an addition to fcflow.h in a header of its own.  The ABI version stays 10, nothing
 * declared in fcflow.h or fcflow_attention_mass.h changes; the conventions are those of fcflow.h (no allocation inside a flow call,
 * an explicit stream, an int status with the cause in the last-error text).
 *
 * Every flow entry of fcflow.h takes one M for the whole batch: ctx is [B, M, E] and all B scenes attend over M context points.
 * The entries below take the same padded batch plus ctx_counts, a DEVICE array [B] of int32: scene b attends over its first
 * ctx_counts[b] context rows only, as if it had been passed alone with ctx[b, :ctx_counts[b]].  Rows ctx_counts[b] .. M-1 of a scene
 * are padding: they are never keys, and what they hold (zeros, NaN, anything) changes neither the result nor whether the pass is
 * repeated on the bf16 limbs.  The library cannot validate a device array without a synchronisation, so the kernels clamp every count
 * into [1, M]; a caller that wants out-of-range counts refused checks them first (the Python binding does).  A scene with few keys does
 * less work: its workgroups run ceil(count / tile) key tiles (csrc/attention.hip).
 * Outputs keep their dense shapes: an attention-weights row and an attention-mass row have M columns, and columns >= ctx_counts[b]
 * are written as exact 0.0f.
 * The entries refuse, with FC_ERR_INVALID and their name in the message, a NULL ctx_counts (use the entries of fcflow.h) and a flow
 * with a global context (ctx is per target point there, [B, N, E]: there is nothing ragged about it). */
#ifndef FCFLOW_CONTEXT_COUNTS_H
#define FCFLOW_CONTEXT_COUNTS_H

#include "fcflow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fc_flow_logprob_f32 with ctx_counts behind ctx.  Workspace: fc_flow_workspace_bytes(flow, B, N, M). */
int fc_flow_logprob_counts_f32(fc_flow* flow, const float* x, const float* ctx, const int32_t* ctx_counts, const float* extra,
                               const float* const* eps, int32_t n_eps, float* logprob, float* z_out, int32_t B, int32_t N, int32_t M,
                               void* workspace, size_t workspace_bytes, void* stream);

/* fc_flow_attention_weights_f32 with ctx_counts behind ctx: out[i] stays [B, P, M]; row p of scene b sums to 1 over its first
 * ctx_counts[b] columns and is 0.0f beyond.  Workspace: fc_flow_workspace_bytes(flow, B, N, M). */
int fc_flow_attention_weights_counts_f32(fc_flow* flow, const float* x, const float* ctx, const int32_t* ctx_counts, const float* extra,
                                         const float* const* eps, int32_t n_eps, const int32_t* layers, int32_t n_layers,
                                         const int32_t* sel, int32_t P, int32_t sel_per_scene, float* const* out, float* logprob,
                                         int32_t B, int32_t N, int32_t M, void* workspace, size_t workspace_bytes, void* stream);

/* fc_flow_attention_mass_f32 (fcflow_attention_mass.h) with ctx_counts behind ctx: out[i] stays [B, M], 0.0f in columns >=
 * ctx_counts[b].  Workspace: fc_flow_attention_mass_workspace_bytes(flow, B, N, M). */
int fc_flow_attention_mass_counts_f32(fc_flow* flow, const float* x, const float* ctx, const int32_t* ctx_counts, const float* extra,
                                      const float* const* eps, int32_t n_eps, const int32_t* layers, int32_t n_layers,
                                      const float* row_weight, float* const* out, float* logprob, int32_t B, int32_t N, int32_t M,
                                      void* workspace, size_t workspace_bytes, void* stream);

/* fc_op_attention_f32 with counts: out[b] = softmax(q[b] k[b, :ctx_counts[b]]^T * scale) v[b, :ctx_counts[b]], q / out [B,N,D],
 * k / v [B,M,D], D in {32, 64, 128, 256}; the kernel is chosen as fc_op_attention_f32 chooses it.  Synchronises the stream. */
int fc_op_attention_counts_f32(const float* q, const float* k, const float* v, float* out, const int32_t* ctx_counts, int32_t B,
                               int32_t N, int32_t M, int32_t D, float scale, void* stream);

/* The same with ONE tensor c [B,M,D] as keys and values, D in {32, 64}, on the kernels of the folded flow engine: one limb image of
 * c, then the shared-tile kernel at D = 64 (the two-image kernel on that image at 32).  Operands 16-byte aligned.  Synchronises. */
int fc_op_attention_ctx_counts_f32(const float* q, const float* c, float* out, const int32_t* ctx_counts, int32_t B, int32_t N,
                                   int32_t M, int32_t D, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FCFLOW_CONTEXT_COUNTS_H */
