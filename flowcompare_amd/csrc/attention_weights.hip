// Softmax rows of the flow's cross attention for selected queries (fc_flow_attention_weights_f32, fc_op_attention_weights_f32):
//   w[b, p, j] = softmax_j( q[b, sel[b,p], :] . k[b, j, :] )      j < M          (models/perceiver.py:108-111, `attn_weights`)
// The forward's kernels (attention.hip) stream the softmax and never form a row; this kernel is launched next to them, only at the layers a
// caller asks about, and reads the operands in the forms the forward leaves them in:
//   K  KF 0: an fp32 panel (head dims 128 and 256, the range-fallback pass, fc_op_*);  KF 1: columns of the stacked K|V GEMM's one-accumulator limb image
//      (GemmEpi::C16 with c16_scale = kOneAccActScale: [16 columns: hi 16 | lo 16] tiles, k 16 = hi + lo) -- joined back to fp32 while the tile
//      is staged, which is exact: hi + lo spans at most 22 significant bits; with k16_rows the folded engine's context image instead, packed rows
//      [key][hi DH | lo DH] of the same form (launch_context_limbs: the keys of EVERY layer, with q carrying the layer's Wk);
//   q  final, or the un-normalised projection of the LayerNorm -> q fold, finished on load with rstd and the bias exactly as attn16_kernel does.
// Arithmetic: fp32 operands on v_mfma_f32_32x32x2_f32, fp32 everywhere (DESIGN.md section 11b says why not the limb products).
//
// One workgroup = 128 selected queries of one scene (4 waves x 32), key tiles of 64 staged in LDS and shared by the waves.  S^T = K Q^T in the
// swapped form of attn_kernel: the query sits on the LANE, its 32 keys of a block in the 16 accumulator registers x 2 half-waves, so a row's
// maximum and sum are in-lane reductions plus one cross-half exchange -- and a row's bits depend on its own query and the keys only, never
// on which other queries share the wave.  Two passes over the key tiles: pass 1 keeps the running maximum m and sum l, pass 2 recomputes S
// and stores exp2(S - m) * (1 / l).  A wave's 32 x 64 block of weights goes through LDS so that every store instruction writes one row's 64
// consecutive floats (a per-lane store at the row pitch would touch 32 lines per instruction).  Keys beyond M are clamped on load, masked to
// -inf before the maximum and never stored; the pad rows of the K panel are never read.
// The operands, the q fragment, the staged tile, the scores and pass 1 live in attention_rows.h, which attention_mass.hip shares.
#include "attention_rows.h"
#include "launch.h"
#include <cstdio>

namespace fc {

struct AttnWParams : AttnRowParams {
    float* out;                          // [B][P][M]
};

// CNT 1: per-scene key counts (AttnProblem::m_counts).  A template parameter, not a null test: with the count read at run time the shipped
// attn_weights_kernel<64, 1> went from 92 to 97 VGPRs and from 4 to 3 waves per SIMD; CNT 0 compiles as before.
template <int DH, int KF, int CNT>
__device__ __forceinline__ void attn_weights_body(const AttnWParams& p) {
    extern __shared__ float smem[];
    AttnRows<DH, KF> rows(p, smem, CNT ? attn_scene_keys(p.m_counts, blockIdx.y, p.M) : p.M);
    constexpr int PL = AttnRows<DH, KF>::PL;
    float* const sP = rows.sP;
    const int lane = rows.lane, li = rows.li, b = rows.b, p0 = rows.p0;
    rows.load_q();

    const int Mb = rows.Mb, ntiles = (Mb + 63) / 64;          // (per-scene key counts: a scene with few keys runs few tiles)
    float m_run, l_run;
    rows.pass1(ntiles, m_run, l_run);
    const float inv_l = 1.0f / l_run;

    // ---- pass 2: the weights, a wave's [32 queries][64 keys] block through LDS, one row segment per store instruction
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();
        rows.stage(t);
        __syncthreads();
        floatx16 s[2];
        rows.scores(t, s);
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                sP[li * PL + rows.tile_key(h2, r)] = __builtin_amdgcn_exp2f(s[h2][r] - m_run) * inv_l;
        __syncthreads();
        const int key = t * 64 + lane;
        if (key < p.M) {
            const int nrow = p.P - p0 < 32 ? p.P - p0 : 32;                 // (wave-uniform; <= 0 for a wave beyond the selection)
            float* op = p.out + ((size_t)b * p.P + p0) * p.M + key;
            for (int rr = 0; rr < nrow; ++rr) op[(size_t)rr * p.M] = !CNT || key < Mb ? sP[rr * PL + lane] : 0.f;
        }
    }
    // ---- columns beyond the scene's last tile: the dense [B][P][M] row ends in exact zeros
    if constexpr (CNT) {
        for (int key = ntiles * 64 + lane; key < p.M; key += 64) {
            const int nrow = p.P - p0 < 32 ? p.P - p0 : 32;
            float* op = p.out + ((size_t)b * p.P + p0) * p.M + key;
            for (int rr = 0; rr < nrow; ++rr) op[(size_t)rr * p.M] = 0.f;
        }
    }
}
template <int DH, int KF>
__global__ __launch_bounds__(256) void attn_weights_kernel(const AttnWParams p) { attn_weights_body<DH, KF, 0>(p); }
template <int DH, int KF>
__global__ __launch_bounds__(256) void attn_weights_counts_kernel(const AttnWParams p) { attn_weights_body<DH, KF, 1>(p); }

template <int DH, int KF>
static void launch_attnw_dh(const AttnWParams& p, int B, hipStream_t s) {
    constexpr size_t lds = attn_rows_lds_bytes<DH>();      // 67 KB at head dim 128, 100 KB at 256
    char name[80];
    const double flops = 4.0 * B * (double)p.P * (double)p.M * DH, bytes = 4.0 * B * (double)p.P * (double)p.M;      // two passes of Q K^T; the output bytes
    snprintf(name, sizeof name, "void fc::attn_weights_%skernel<%d, %d>(fc::AttnWParams)", p.m_counts ? "counts_" : "", DH, KF);
    if (p.m_counts) launch_kernel<attn_weights_counts_kernel<DH, KF>, (int)lds>(name, flops, bytes, dim3((p.P + 127) / 128, B), dim3(256), lds, s, p);
    else launch_kernel<attn_weights_kernel<DH, KF>, (int)lds>(name, flops, bytes, dim3((p.P + 127) / 128, B), dim3(256), lds, s, p);
}

int attn_rows_params(const char* what, const AttnQuery& qy, const AttnKeys& kv, const AttnProblem& pb, AttnRowParams& p) {
    const std::string w = std::string(what) + ": ";
    const int dh_pad = pb.dh_pad;
    const bool limbs = kv.form != AttnKeys::PANELS;
    if (pb.B <= 0 || pb.N <= 0 || pb.M <= 0) throw Error(FC_ERR_INVALID, w + "empty problem");
    if (!qy.q || (limbs ? !kv.img : !kv.k)) throw Error(FC_ERR_INVALID, w + "null pointer");
    if (qy.ldq % 4 != 0 || ((uintptr_t)qy.q & 15)) throw Error(FC_ERR_INVALID, w + "q must be 16-byte aligned with a pitch that is a multiple of 4 floats");
    p.q = qy.q; p.ldq = qy.ldq;
    p.N = pb.N; p.n_stride = pb.n_stride_rows; p.M = pb.M; p.m_stride = pb.m_stride_rows; p.qscale = qy.qscale; p.m_counts = pb.m_counts;
    if (const AttnLnq* l = qy.lnq) { p.q_sumsq = l->sumsq; p.q_slots = l->slots; p.q_pitch = l->pitch; p.q_inv_width = l->inv_width; p.q_bias = l->bias; }
    if (limbs) {
        if (kv.form == AttnKeys::CONTEXT) {
            if (((uintptr_t)kv.img & 15)) throw Error(FC_ERR_INVALID, w + "the context limb image must be 16-byte aligned");
            p.k16 = kv.img;
            p.ld16 = 2 * dh_pad;
            p.k16_rows = 1;
        } else {
            if (kv.col0 % 16 != 0 || kv.n_pad % 16 != 0 || dh_pad > 64) throw Error(FC_ERR_INVALID, w + "limb-image K needs 16-column tiles and head dim <= 64");
            p.k16 = kv.img + (size_t)(kv.col0 / 16) * 32;
            p.ld16 = kv.n_pad * 2;
        }
        if (dh_pad != 32 && dh_pad != 64) throw Error(FC_ERR_UNSUPPORTED, w + "inner dim (padded) must be 32 or 64 with a limb-image K");
        return 1;
    }
    if (kv.ldk % 4 != 0 || ((uintptr_t)kv.k & 15)) throw Error(FC_ERR_INVALID, w + "k must be 16-byte aligned with a pitch that is a multiple of 4 floats");
    p.k = kv.k; p.ldk = kv.ldk;
    if (dh_pad != 32 && dh_pad != 64 && dh_pad != 128 && dh_pad != 256) throw Error(FC_ERR_UNSUPPORTED, w + "inner dim (padded) must be 32, 64, 128 or 256");
    return 0;
}

void launch_attention_weights(const AttnQuery& qy, const AttnKeys& kv, const AttnProblem& pb, const int32_t* sel, int P, int sel_per_scene,
                              float* out, hipStream_t s) {
    const int B = pb.B;
    if (P <= 0) throw Error(FC_ERR_INVALID, "attention weights: empty problem");
    if (!out) throw Error(FC_ERR_INVALID, "attention weights: null pointer");
    if (!sel && P != pb.N) throw Error(FC_ERR_INVALID, "attention weights: without a selection table P must equal N");
    AttnWParams p{};
    const int kf = attn_rows_params("attention weights", qy, kv, pb, p);
    p.out = out; p.sel = sel; p.sel_stride = sel && sel_per_scene ? P : 0; p.P = P;
    if (kf) {
        if (pb.dh_pad == 32) launch_attnw_dh<32, 1>(p, B, s);
        else launch_attnw_dh<64, 1>(p, B, s);
        return;
    }
    switch (pb.dh_pad) {
        case 32: launch_attnw_dh<32, 0>(p, B, s); break;
        case 64: launch_attnw_dh<64, 0>(p, B, s); break;
        case 128: launch_attnw_dh<128, 0>(p, B, s); break;
        default: launch_attnw_dh<256, 0>(p, B, s); break;
    }
}

}  // namespace fc
