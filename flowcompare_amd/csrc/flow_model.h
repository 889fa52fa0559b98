// fc_flow's packed model: what flow_pack.cpp builds once at fc_flow_create and flow_engine.cpp's launch schedule reads on every call.
#pragma once
#include <algorithm>

#include "hostpack.h"

namespace fc {

struct AttnPack {
    PackedLinear q;      // LN-folded, pre-scaled q projection  [I_pad][A_in_pad]
    MatD q_w;            // the same folded matrix / bias on the host (double), for the LayerNorm -> q fold below
    VecD q_b;
    // LayerNorm folded THROUGH the (activation-free) pre-MLP out_layer: rows [0, A_in) = mean-centred out_layer (its outputs are only
    // squared and summed per row), rows [A_in, A_in + I_pad) = q projection of the centred outputs; q = q_unnorm * rstd + q_bias
    PackedLinear lnq;
    float* q_bias = nullptr;
    bool has_lnq = false;
    MatD lin_w;          // [attn_dim][I]  (folded into the consumer's in_layer; with the K|V fold: Wlin Wv, [attn_dim][E])
    VecD lin_b;
    int kv_col = 0;      // column of this layer's [K | V] block inside the kv buffer (unused with the K|V fold)
};

// CIFblock pieces (models/cif_block.py:49-112), all expressed in the NATURAL index order of x (D) and z2 (Dc - D): the two
// Reverse permutations are folded into the packed weights' row / column maps.
struct CifPack {
    PackedMLP dist;               // shared ConditionalNormal net of augmenter and slicer: x (x layout) -> [mean | log_std] pairs
    PackedMLP aff;                // affine_cif: flip(z2) -> (s, t) for flip(x); t rows carry the x-part ActNorm
    float* post_scale = nullptr;  // g[k] = exp(-log_scale) of the x part (behind s)
    float* z2_shift = nullptr;    // ActNorm of the z2 part: v = (z2 - shift) * scale
    float* z2_scale = nullptr;
    double log_const = 0.0;       // data-independent log-det of the CIF ActNorm
};

struct BlockPack {
    bool has_attn = false;
    PackedMLP pre;       // pre_attention_mlp
    AttnPack attn;
    PackedMLP net;       // coupling MLP (in_layer has the folded context segment)
    float* expm_scal = nullptr;   // ExponentialCoupling: {scale, shift, rescale, reshift}
    bool has_cif = false;
    CifPack cif;
    bool has_lin = false;
    PackedLinear lin;    // folded ActNorm + permuter (absent after the last block)
    MatD lin_w;          // host copy (double) for the lazily built inverse
    VecD lin_b;
    bool has_lin_inv = false;
    PackedLinear lin_inv;
    double log_const = 0.0;       // data-independent log-dets of this block's ActNorm + permuter
};

struct Dims {
    int Din, D, d1, d2, d1_pad, d2_pad, ldx;
    int E, E_pad, X;
    int A_in = 0, A_in_pad = 0, I = 0, I_pad = 0;
    int H_pad = 0;       // widest hidden activation
    int ldp = 0;         // spline / expm parameter pitch
    int Dc = 0, nz = 0, nz_pad = 0;   // CIF: cif_latent_dim, Dc - D
    int ldh() const { return std::max(H_pad, 32); }   // pitch of the hidden activation buffers (FlowWs::h, h16)
};

}  // namespace fc

struct fc_flow {
    int* fp16_flag = nullptr;   // device word raised by the split-fp16 GEMM loop on an activation >= 65504 (common.h: Fp16Guard)
    int* expm_status = nullptr; // device word raised by the wide ExponentialCoupling kernel on a matrix beyond its bound (expm_wide.hip)
    fc_flow_config cfg;
    fc::Dims d;
    fc::DeviceArena arena;
    bool has_augment = false;
    fc::PackedMLP aug_pre, aug_net;
    fc::AttnPack aug_attn;
    std::vector<fc::BlockPack> blocks;
    fc::PackedLinear kv_all;   // ctx -> [K|V] of every attention (augmenter first); not packed when kv_fold
    bool kv_fold = false;      // to_kv folded into the q projections and the consumers' in_layers: keys = values = the context panel
    int n_attn = 0;
    double log_const = 0.0;
};

namespace fc {

// flow_pack.cpp
void build_flow(fc_flow& f, const WeightTable& wt);                        // everything fc_flow_create packs; launches nothing
bool kv_fold_gate_dims(int E, int inner, bool q_bias, bool kv_bias);       // the K|V fold's gate on the shapes alone (fc_debug_kv_fold_gate)
void ensure_lin_inverse(fc_flow& f);                                       // packs the blocks' inverted ActNorm + permuter on the first inverse pass
// the pieces of an attention's query side that build_flow and the single-chain test entry (ops_api.cpp fc_debug_premlp_q_f32) both pack with
int pad_inner(int I);                                                      // q columns of an inner width: 32, 64, 128 or 256
void fold_q_projection(const WeightTable& wt, const std::string& to_q, const std::string& norm, MatD& wq, VecD& bq);   // gamma, beta, I^-0.5, log2 e -> to_q (double)
void pack_q_projection(DeviceArena& arena, const MatD& wq, const VecD& bq, const Dims& d, AttnPack& out);              // AttnPack::q, q_w, q_b
void build_lnq(DeviceArena& arena, const Dims& d, const WeightTable& wt, const std::string& out_prefix, AttnPack& at);  // AttnPack::lnq where the shapes allow it
// flow_engine.cpp
void flow_set_trace(float* buf, size_t floats);                            // fc_debug_flow_trace
void flow_set_expm_info(float* buf, size_t floats);                        // fc_debug_expm_info

// d2 > 16: the coupling runs on the matrix-exponential action kernel (expm_wide.hip) and owns a status word
inline bool expm_wide(const fc_flow& f) { return f.cfg.flow_type == FC_FLOW_EXPONENTIAL && f.d.d2 > kExpmSmallMaxD2; }

}  // namespace fc
