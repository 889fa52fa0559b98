// fc_flow, the create-time half: the checkpoint's tensors -> the packed model of flow_model.h.  Double-precision algebra and pack_linear only;
// flow_engine.cpp is the launch schedule that reads the result.
//
// Reference being replaced: models.Flow.log_prob (models/transform.py:70-76) over the transform list that
// initialize_flow assembles (model_initialization.py:136-160).  Weight folding done once at create (double precision):
//   * attn.fn.lin (I -> attn_dim) is folded INTO the coupling / augmenter in_layer:  W_ctx (W_lin a + b_lin) = (W_ctx W_lin) a + W_ctx b_lin
//   * LayerNorm gamma/beta, the softmax scale inner^-0.5 and log2(e) are folded into the q projection
//   * to_kv away (kv_fold_gate below): q k^T = LN(h) (Wk^T Wq)^T ctx^T and lin(softmax v) = (softmax ctx) (Wlin Wv)^T + b, so Wk rides in the q
//     projection, Wv in lin (and with it in the consumer's in_layer), and every attention's keys AND values are the context panel itself
//   * ActNorm and the permuter (LinearLU: L U; FullCombiner: w; ExponentialCombiner: expm; Permuter: P) become ONE matrix
//     z = W' x + b',  W' = P diag(e^-log_scale),  b' = -W' shift; their log-dets are data independent and summed into one constant
//   * extra context (one scalar per scene) enters every in_layer as a rank-1 epilogue term instead of a concatenated column
// Activation layout in HBM: x is [rows, d1_pad + d2_pad] = [x1 | 0-pad | x2 | 0-pad] (pads kept zero by construction), every
// other activation is [rows, round_up(width, 32)]; rows are padded to 256.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <exception>
#include <mutex>
#include <thread>

#include "flow_model.h"
#include "spline.h"

namespace fc {

// The K|V fold keeps every weight shape only when the context embedding is as wide as the attention's inner dimension (every shipped
// configuration: 64 = 64), and the algebra above has no place for a bias on to_q / to_kv (the reference has none, models/perceiver.py:89-95).
// The attention kernels then read the context panel (pitch E_pad = E rounded up to 32) as I_pad-column keys and values, so the two padded
// widths must agree as well: inner 65..96 pads to 128 (pad_inner) but its panel to 96, and keeps the projection.
int pad_inner(int I) {
    if (I <= 32) return 32;
    if (I <= 64) return 64;
    if (I <= 128) return 128;
    if (I <= 256) return 256;
    throw Error(FC_ERR_UNSUPPORTED, "attention inner dim (cross_heads*cross_dim_head) > 256 is not supported (the limit is 256)");
}
bool kv_fold_gate_dims(int E, int inner, bool q_bias, bool kv_bias) {
    return E > 0 && E == inner && inner <= 128 && round_up(E, 32) == pad_inner(inner) && !q_bias && !kv_bias;
}
static bool kv_fold_gate(const fc_flow_config& c, const WeightTable& wt, const std::vector<std::string>& attn_prefixes) {
    if (!g_knobs.kv_fold || attn_prefixes.empty()) return false;      // (knob 33)
    for (const std::string& p : attn_prefixes) {
        const HostTensor& wq = wt.get(p + ".fn.attention.to_q.weight");
        if (wq.shape.size() != 2 || !kv_fold_gate_dims(c.input_embedding_dim, (int)wq.shape[0], wt.has(p + ".fn.attention.to_q.bias"),
                                                       wt.has(p + ".fn.attention.to_kv.bias")))
            return false;
    }
    return true;
}

// q' = c * Wq (gamma . n + beta),  c = inner^-0.5 * log2(e)   (models/perceiver.py:18-26, 96-110): `to_q`.weight [I, A_in] with LayerNorm `norm`'s
// gamma / beta, the softmax scale and log2 e folded in, and the bias that beta leaves behind -- in double, nothing packed yet
void fold_q_projection(const WeightTable& wt, const std::string& to_q, const std::string& norm, MatD& wq, VecD& bq) {
    const HostTensor& wq_t = wt.get(to_q + ".weight");
    if (wq_t.shape.size() != 2) throw Error(FC_ERR_SHAPE, to_q + ".weight must be 2-D");
    const int I = (int)wq_t.shape[0], A_in = (int)wq_t.shape[1];
    wq = mat_from(wq_t);
    VecD gamma = vec_from(wt.get(norm + ".weight", {A_in})), beta = vec_from(wt.get(norm + ".bias", {A_in}));
    const double c = std::pow((double)I, -0.5) * kLog2e;
    bq.assign(I, 0.0);
    for (int i = 0; i < I; ++i)
        for (int k = 0; k < A_in; ++k) {
            bq[i] += c * wq.at(i, k) * beta[k];
            wq.at(i, k) *= c * gamma[k];
        }
}
// the folded projection (fold_q_projection, then the K|V fold where it applies) as the attention's packed q layer, with its host copy for build_lnq
void pack_q_projection(DeviceArena& arena, const MatD& wq, const VecD& bq, const Dims& d, AttnPack& out) {
    out.q = pack_linear(arena, wq, bq, {}, map_prefix(wq.rows, d.I_pad), map_prefix(wq.cols, d.A_in_pad), {d.A_in_pad});
    out.q_w = wq;
    out.q_b = bq;
}

static void build_attn(fc_flow& f, const WeightTable& wt, const std::string& p, AttnPack& out, std::vector<MatD>& kv_rows, int slot) {
    Dims& d = f.d;
    MatD wq;
    VecD bq;
    fold_q_projection(wt, p + ".fn.attention.to_q", p + ".norm", wq, bq);
    const int I = wq.rows, A_in = wq.cols;
    if (d.I == 0) { d.I = I; d.I_pad = pad_inner(I); d.A_in = A_in; d.A_in_pad = round_up(A_in, 32); }
    if (I != d.I || A_in != d.A_in) throw Error(FC_ERR_SHAPE, p + ": all attention blocks must share inner / input dims");
    const HostTensor& wkv_t = wt.get(p + ".fn.attention.to_kv.weight", {2 * I, d.E});
    MatD wkv = mat_from(wkv_t);                 // rows [0,I) = K, [I,2I) = V  (chunk(2, dim=-1))
    const HostTensor& wl = wt.get(p + ".fn.lin.weight");
    if (wl.shape.size() != 2 || wl.shape[1] != I) throw Error(FC_ERR_SHAPE, p + ".fn.lin.weight: expected [attn_dim, inner]");
    out.lin_w = mat_from(wl);
    out.lin_b = vec_from(wt.get(p + ".fn.lin.bias", {wl.shape[0]}));
    if (f.kv_fold) {
        // q . k = (Wq' n + bq') . (Wk ctx) = ctx . (Wk^T Wq' n + Wk^T bq'): the q projection now ends in the E (= I) context columns;
        // Wlin (P Wv ctx) = (Wlin Wv) (P ctx): lin now starts from them.  Shapes unchanged (kv_fold_gate).
        MatD wq2(d.E, A_in), lw2(out.lin_w.rows, d.E);
        VecD bq2(d.E, 0.0);
        for (int e = 0; e < d.E; ++e) {
            for (int i = 0; i < I; ++i) {
                const double wk = wkv.at(i, e);
                bq2[e] += wk * bq[i];
                for (int k = 0; k < A_in; ++k) wq2.at(e, k) += wk * wq.at(i, k);
            }
        }
        for (int c2 = 0; c2 < out.lin_w.rows; ++c2)
            for (int i = 0; i < I; ++i) {
                const double wlv = out.lin_w.at(c2, i);
                for (int e = 0; e < d.E; ++e) lw2.at(c2, e) += wlv * wkv.at(I + i, e);
            }
        wq = wq2; bq = bq2; out.lin_w = lw2;
    } else {
        MatD blk(2 * d.I_pad, d.E);
        for (int i = 0; i < I; ++i)
            for (int k = 0; k < d.E; ++k) { blk.at(i, k) = wkv.at(i, k); blk.at(d.I_pad + i, k) = wkv.at(I + i, k); }
        out.kv_col = slot * 2 * d.I_pad;            // column block of this attention in the stacked K|V projection
        kv_rows[slot] = blk;
    }
    pack_q_projection(f.arena, wq, bq, d, out);
}

// LayerNorm -> q fold (see AttnPack::lnq).  h = W3 a + b3 has no activation, so its centred form h_c = h - mean(h) is linear in a:
// W3c = W3 - 1 (1^T W3)/A_in, b3c = b3 - mean(b3).  LayerNorm(h) = h_c / sigma (gamma, beta live in the q projection), hence
// q = Wq' h_c / sigma + bq' = (Wq' W3c a + Wq' b3c) / sigma + bq' with sigma^2 = mean(h_c^2) + eps.  One GEMM with N = A_in + I_pad
// columns yields h_c (only squared and summed per row in the epilogue, never stored) and q_unnorm; lnq_finalize_kernel applies
// rstd and bq'.  Replaces out_layer's store, the LayerNorm pass and the q projection GEMM.
void build_lnq(DeviceArena& arena, const Dims& d, const WeightTable& wt, const std::string& out_prefix, AttnPack& at) {
    const HostTensor& w_t = wt.get(out_prefix + ".weight");
    const MatD w3 = mat_from(w_t);
    const int A = w3.rows, K = w3.cols;
    if (A != d.A_in || d.A_in != d.A_in_pad || d.A_in % 64 != 0 || d.I_pad != 64 || K % 32 != 0) return;     // shapes the fused epilogue handles
    const VecD b3 = vec_from(wt.get(out_prefix + ".bias", {A}));
    MatD m(A + d.I_pad, K);
    VecD bias(A + d.I_pad, 0.0);
    double bmean = 0.0;
    for (int o = 0; o < A; ++o) bmean += b3[o] / A;
    for (int k = 0; k < K; ++k) {
        double cm = 0.0;
        for (int o = 0; o < A; ++o) cm += w3.at(o, k) / A;
        for (int o = 0; o < A; ++o) m.at(o, k) = w3.at(o, k) - cm;
    }
    for (int o = 0; o < A; ++o) bias[o] = b3[o] - bmean;
    for (int i = 0; i < at.q_w.rows; ++i) {
        for (int k = 0; k < K; ++k) {
            double acc = 0.0;
            for (int o = 0; o < A; ++o) acc += at.q_w.at(i, o) * m.at(o, k);
            m.at(A + i, k) = acc;
        }
        double acc = 0.0;
        for (int o = 0; o < A; ++o) acc += at.q_w.at(i, o) * bias[o];
        bias[A + i] = acc;
    }
    at.lnq = pack_linear(arena, m, bias, {}, map_prefix(A + d.I_pad, A + d.I_pad), map_prefix(K, K), {K});
    std::vector<float> qb(d.I_pad, 0.f);
    for (int i = 0; i < at.q_w.rows; ++i) qb[i] = (float)at.q_b[i];
    at.q_bias = arena.upload(qb);
    at.has_lnq = at.lnq.W2 != nullptr;
}

// in_layer over cat(first(n_first), extra(X), ctxvec(C)) -> packed [first_pad | second_pad] + rank-1 extra column.
// With attention the context segment is the folded attention output (I_pad wide); in global mode it is the E-wide embedding.
static PackedLinear build_in_layer(fc_flow& f, const WeightTable& wt, const std::string& prefix, int n_first, int first_pad,
                                   const AttnPack* attn) {
    Dims& d = f.d;
    const HostTensor& wt_in = wt.get(prefix + ".in_layer.weight");
    MatD w = mat_from(wt_in);
    const int H = w.rows;
    VecD b = vec_from(wt.get(prefix + ".in_layer.bias", {H}));
    const int C = attn ? attn->lin_w.rows : d.E;
    if (w.cols != n_first + d.X + C) throw Error(FC_ERR_SHAPE, prefix + ".in_layer.weight: expected input width " +
                                                                  std::to_string(n_first + d.X + C) + ", got " + std::to_string(w.cols));
    const int c0 = n_first + d.X;
    const int second = attn ? d.I : d.E, second_pad = attn ? d.I_pad : d.E_pad;
    MatD fw(H, n_first + second);
    VecD colvec;
    if (d.X) colvec.assign(H, 0.0);
    for (int n = 0; n < H; ++n) {
        for (int k = 0; k < n_first; ++k) fw.at(n, k) = w.at(n, k);
        if (d.X) colvec[n] = w.at(n, n_first);
        if (attn) {
            for (int j = 0; j < d.I; ++j) {
                double s = 0;
                for (int c = 0; c < C; ++c) s += w.at(n, c0 + c) * attn->lin_w.at(c, j);
                fw.at(n, n_first + j) = s;
            }
            double sb = 0;
            for (int c = 0; c < C; ++c) sb += w.at(n, c0 + c) * attn->lin_b[c];
            b[n] += sb;
        } else {
            for (int c = 0; c < C; ++c) fw.at(n, n_first + c) = w.at(n, c0 + c);
        }
    }
    std::vector<int> k2(second_pad, -1);
    for (int j = 0; j < second; ++j) k2[j] = n_first + j;
    return pack_linear(f.arena, fw, b, colvec, map_prefix(H, round_up(H, 32)), map_concat({map_prefix(n_first, first_pad), k2}),
                       {first_pad, second_pad});
}

// One pre-conditioner (augmenter or flow layer): its attention, the pre-attention MLP `pm` reading n_in (padded in_pad) columns, and the
// LayerNorm -> q fold through that MLP's out_layer.
static void build_precond(fc_flow& f, const WeightTable& wt, const std::string& attn_prefix, const std::string& pm, int n_in, int in_pad,
                          PackedMLP& pre, AttnPack& at, std::vector<MatD>& kv_rows, int slot) {
    build_attn(f, wt, attn_prefix, at, kv_rows, slot);
    pack_mlp_mid(f.arena, wt, pm, pre);
    pre.in_layer = pack_plain_linear(f.arena, wt, pm + ".in_layer", n_in, in_pad);
    pre.out_layer = pack_plain_linear(f.arena, wt, pm + ".out_layer", pre.sizes.back(), round_up(pre.sizes.back(), 32));
    if (pre.out_layer.N_pad != f.d.A_in_pad) throw Error(FC_ERR_SHAPE, pm.substr(pm.rfind('.') + 1) + " output width != attn_input_dim");
    build_lnq(f.arena, f.d, wt, pm + ".out_layer", at);
}

// out_layer of a ConditionalNormal net `pn` over nz noise dims, pair-packed [mean 32 | log_std 32] (EPI_AUGMENT / EPI_SLICE)
static void build_pairs_out_layer(fc_flow& f, const WeightTable& wt, const std::string& pn, int nz, PackedMLP& net) {
    const int hl = net.sizes.back();
    const HostTensor& wo = wt.get(pn + ".out_layer.weight", {2 * nz, hl});
    net.out_layer = pack_linear(f.arena, mat_from(wo), vec_from(wt.get(pn + ".out_layer.bias", {2 * nz})), {}, map_pairs(nz, nz),
                                map_prefix(hl, round_up(hl, 32)), {round_up(hl, 32)});
}

// ActNorm (models/act_norm.py:37-43) followed by the permuter (models/permuters.py) as one affine map on the x layout.
static void build_lin(fc_flow& f, const WeightTable& wt, int idx_actnorm, int idx_perm, BlockPack& blk) {
    const Dims& d = f.d;
    const int D = d.D;
    VecD shift(D, 0.0), ls(D, 0.0);
    if (idx_actnorm >= 0) {
        const std::string p = "transforms." + std::to_string(idx_actnorm);
        shift = vec_from(wt.get(p + ".shift", {1, D}));
        ls = vec_from(wt.get(p + ".log_scale", {1, D}));
        for (double v : ls) blk.log_const -= v;
    }
    const std::string p = "transforms." + std::to_string(idx_perm);
    MatD Wp(D, D);
    switch (f.cfg.permuter_type) {
        case FC_PERM_LINEAR_LU: {
            const int ntri = D * (D - 1) / 2;
            const HostTensor& lo = wt.get(p + ".lower_entries", {ntri});
            const HostTensor& up = wt.get(p + ".upper_entries", {ntri});
            const HostTensor& ud = wt.get(p + ".unconstrained_upper_diag", {D});
            MatD L(D, D), U(D, D);
            int t = 0;
            for (int i = 0; i < D; ++i) { for (int j = 0; j < i; ++j) L.at(i, j) = lo.data[t++]; L.at(i, i) = 1.0; }
            t = 0;
            for (int i = 0; i < D; ++i) for (int j = i + 1; j < D; ++j) U.at(i, j) = up.data[t++];
            for (int i = 0; i < D; ++i) {
                const double dg = softplus_d(ud.data[i]) + (double)f.cfg.linear_lu_eps;
                U.at(i, i) = dg;
                blk.log_const += std::log(dg);
            }
            Wp = matmul(L, U);               // z = L (U x)   (permuters.py:164-169)
            break;
        }
        case FC_PERM_RANDOM: {
            const HostTensor& pm = wt.get(p + ".permutation", {D});
            for (int i = 0; i < D; ++i) {
                const int src = (int)std::lround(pm.data[i]);
                if (src < 0 || src >= D) throw Error(FC_ERR_INVALID, p + ".permutation out of range");
                Wp.at(i, src) = 1.0;          // y = x.index_select(-1, permutation)
            }
            break;
        }
        case FC_PERM_FULL: {
            Wp = mat_from(wt.get(p + ".w", {D, D}));
            blk.log_const += slogdet_abs(Wp);
            break;
        }
        case FC_PERM_EXPONENTIAL: {
            MatD w = mat_from(wt.get(p + ".w", {D, D}));
            const double sc = wt.get(p + ".scale", {1}).data[0], sh = wt.get(p + ".shift", {1}).data[0];
            const double rs = wt.get(p + ".rescale", {1}).data[0], rsh = wt.get(p + ".reshift", {1}).data[0];
            for (auto& e : w.v) e = rs * std::tanh(sc * e + sh) + rsh + 1e-8;
            for (int i = 0; i < D; ++i) blk.log_const += w.at(i, i);
            Wp = expm_double(w);
            break;
        }
        default: throw Error(FC_ERR_INVALID, "unknown permuter_type");
    }
    VecD b(D, 0.0);
    for (int i = 0; i < D; ++i) {
        double s = 0;
        for (int k = 0; k < D; ++k) {
            Wp.at(i, k) *= std::exp(-ls[k]);
            s += Wp.at(i, k) * shift[k];
        }
        b[i] = -s;
    }
    const std::vector<int> xl = map_xlayout(d.d1, d.d1_pad, d.d2, d.d2_pad);
    blk.lin = pack_linear(f.arena, Wp, b, {}, xl, xl, {d.ldx});
    blk.has_lin = true;
    blk.lin_w = Wp;
    blk.lin_b = b;
}

static void build_out_layer(fc_flow& f, const WeightTable& wt, const std::string& prefix, PackedMLP& net) {
    Dims& d = f.d;
    const int hl = net.sizes.back();
    const HostTensor& w = wt.get(prefix + ".out_layer.weight");
    const int n = (int)w.shape[0];
    VecD b = vec_from(wt.get(prefix + ".out_layer.bias", {n}));
    std::vector<int> nmap;
    if (f.cfg.flow_type == FC_FLOW_AFFINE) {
        if (n != 2 * d.d2) throw Error(FC_ERR_SHAPE, prefix + ".out_layer: affine coupling expects 2*(D - D/2) outputs");
        nmap = map_pairs(d.d2, d.d2);
    } else if (f.cfg.flow_type == FC_FLOW_SPLINE) {
        const int per = 3 * f.cfg.num_bins_spline + 1;
        if (n != per * d.d1) throw Error(FC_ERR_SHAPE, prefix + ".out_layer: spline coupling expects (3K+1)*(D/2) outputs");
        if (n != per * d.d2) throw Error(FC_ERR_UNSUPPORTED, "spline coupling with odd latent_dim fails in the reference too (reshape)");
        // tile-grouped dim-major output (spline.h): a 128-column GEMM tile holds all 3K+1 parameters of DPT transformed dims, so the
        // workgroup that produced the tile evaluates those splines in its epilogue (reference order is j*(3K+1) + p)
        const int K = f.cfg.num_bins_spline;
        nmap.assign(spline_ncols(d.d2, K), -1);
        for (int j = 0; j < d.d2; ++j)
            for (int pp = 0; pp < per; ++pp) nmap[spline_col(j, pp, K)] = j * per + pp;
    } else {
        if (n != d.d2 * d.d2 + d.d2) throw Error(FC_ERR_SHAPE, prefix + ".out_layer: exponential coupling expects d2^2 + d2 outputs");
        nmap = map_prefix(n, round_up(n, 32));
    }
    net.out_layer = pack_linear(f.arena, mat_from(w), b, {}, nmap, map_prefix(hl, round_up(hl, 32)), {round_up(hl, 32)});
    if (f.cfg.flow_type == FC_FLOW_SPLINE && f.cfg.num_bins_spline == 8) {
        // the one-accumulator image of the 256 x 256 fused spline kernel (spline_wide.hip): rows in that kernel's register-slot order, pre-scaled by
        // the power of two that puts max |w| into [2^14, 2^15).
        // Folded (spline_fold, knob 34): softmax is shift-invariant and the reference never reads derivative logit 8 (models/spline_coupling.py:24-66: F.pad, then
        // both end entries overwritten), so only 22 of a dim's 25 parameters carry information: width and height rows i < 7 become W_i - W_7 with
        // b_i - b_7, rows 7 / 15 / 24 of every dim leave the image.  The subtraction is made in double from the checkpoint's values (the image
        // kernel, from the fp32 pack that holds them exactly); the scale is taken HERE over the same folded rows.  W / W2 / W3 / bias keep all 25.
        const bool fold = g_knobs.spline_fold != 0;      // (knob 34)
        float wmax = 0.f;
        const int hk = (int)w.shape[1];
        for (int r = 0; r < n; ++r) {
            const int pp = r % 25;
            if (fold && (pp == 7 || pp == 15 || pp == 24)) continue;
            const float* wr = w.data + (size_t)r * hk;
            const float* ws = fold && pp < 16 ? w.data + (size_t)(r - pp + (pp < 8 ? 7 : 15)) * hk : nullptr;
            for (int k = 0; k < hk; ++k) wmax = std::max(wmax, std::fabs(ws ? (float)((double)wr[k] - (double)ws[k]) : wr[k]));
        }
        spline_wide_attach(f.arena, net.out_layer, wmax, nullptr, fold);
    }
}

// pair-packed row map from explicit (first-half row, second-half row) lists
static std::vector<int> map_pairs_rows(const std::vector<int>& first, const std::vector<int>& second) {
    const int n = (int)first.size(), np = (n + 31) / 32;
    std::vector<int> m(np * 64, -1);
    for (int j = 0; j < n; ++j) { m[64 * (j / 32) + j % 32] = first[j]; m[64 * (j / 32) + 32 + j % 32] = second[j]; }
    return m;
}

// CIFblock (models/cif_block.py:49-112).  Natural-order algebra (x: D dims, z2: nz = Dc - D dims, Reverse folded away):
//   z2 = mu(x) + eps sigma(x)                                   ldj -= log N(z2)
//   (s,t) = affine_cif.nn(flip(z2)),  zx[k] = (x[k] s'[k] + t'[k] - shift[Dc-1-k]) e^{-log_scale[Dc-1-k]},  s'[k] = s[D-1-k]   ldj += sum log s
//   x2n[j] = (z2[j] - shift[nz-1-j]) e^{-log_scale[nz-1-j]}      ldj += sum(-log_scale)  (constant)
//   ldj += log N(x2n; mu(zx), sigma(zx))                         (Slice with the SAME distribution object)
//   then the attention-conditioned coupling on zx.
static void build_cif(fc_flow& f, const WeightTable& wt, const std::string& p, CifPack& c) {
    Dims& d = f.d;
    const int D = d.D, nz = d.nz, Dc = d.Dc;
    const std::string pd = p + ".augmenter.noise_dist.net";
    if (wt.has(p + ".slicer.noise_dist.net.in_layer.weight")) {          // shared object: both prefixes must hold the same values
        const HostTensor& a = wt.get(pd + ".in_layer.weight");
        const HostTensor& b = wt.get(p + ".slicer.noise_dist.net.in_layer.weight");
        if (a.shape != b.shape || memcmp(a.data, b.data, sizeof(float) * (size_t)a.numel()) != 0)
            throw Error(FC_ERR_INVALID, p + ": augmenter.noise_dist and slicer.noise_dist must be identical (one shared ConditionalNormal)");
    }
    pack_mlp_mid(f.arena, wt, pd, c.dist);
    {
        const HostTensor& w = wt.get(pd + ".in_layer.weight");
        if (w.shape.size() != 2 || w.shape[1] != D) throw Error(FC_ERR_SHAPE, pd + ".in_layer.weight: expected input width latent_dim");
        const int h = (int)w.shape[0];
        c.dist.in_layer = pack_linear(f.arena, mat_from(w), vec_from(wt.get(pd + ".in_layer.bias", {h})), {}, map_prefix(h, round_up(h, 32)),
                                      map_xlayout(d.d1, d.d1_pad, d.d2, d.d2_pad), {d.ldx});
        build_pairs_out_layer(f, wt, pd, nz, c.dist);
    }
    VecD shift = vec_from(wt.get(p + ".act_norm.shift", {1, Dc})), ls = vec_from(wt.get(p + ".act_norm.log_scale", {1, Dc}));
    for (double v : ls) c.log_const -= v;
    std::vector<float> g(gemm_n_alloc(round_up(D, 32) * 2), 0.f), sh2(gemm_n_alloc(round_up(nz, 32) * 2), 0.f), g2(sh2.size(), 1.f);
    for (int k = 0; k < D; ++k) g[k] = (float)std::exp(-ls[Dc - 1 - k]);
    for (int j = 0; j < nz; ++j) { sh2[j] = (float)shift[nz - 1 - j]; g2[j] = (float)std::exp(-ls[nz - 1 - j]); }
    c.post_scale = f.arena.upload(g);
    c.z2_shift = f.arena.upload(sh2);
    c.z2_scale = f.arena.upload(g2);
    const std::string pa = p + ".affine_cif.nn";
    pack_mlp_mid(f.arena, wt, pa, c.aff);
    {
        const HostTensor& w = wt.get(pa + ".in_layer.weight");
        if (w.shape.size() != 2 || w.shape[1] != nz) throw Error(FC_ERR_SHAPE, pa + ".in_layer.weight: expected input width cif_latent_dim - latent_dim");
        const int h = (int)w.shape[0];
        std::vector<int> km(d.nz_pad, -1);
        for (int j = 0; j < nz; ++j) km[j] = nz - 1 - j;                   // input arrives as z2 in natural order; the net saw flip(z2)
        c.aff.in_layer = pack_linear(f.arena, mat_from(w), vec_from(wt.get(pa + ".in_layer.bias", {h})), {}, map_prefix(h, round_up(h, 32)), km, {d.nz_pad});
        const int hl = c.aff.sizes.back();
        MatD wo = mat_from(wt.get(pa + ".out_layer.weight", {2 * D, hl}));
        VecD bo = vec_from(wt.get(pa + ".out_layer.bias", {2 * D}));
        std::vector<int> srow(D), trow(D);
        for (int k = 0; k < D; ++k) {
            const int i = D - 1 - k;                                       // position inside flip(x)
            srow[k] = i; trow[k] = D + i;
            const double gk = std::exp(-ls[Dc - 1 - k]);
            for (int c2 = 0; c2 < hl; ++c2) wo.at(D + i, c2) *= gk;          // t'' = (t - shift) g
            bo[D + i] = (bo[D + i] - shift[Dc - 1 - k]) * gk;
        }
        c.aff.out_layer = pack_linear(f.arena, wo, bo, {}, map_pairs_rows(srow, trow), map_prefix(hl, round_up(hl, 32)), {round_up(hl, 32)});
    }
}

void build_flow(fc_flow& f, const WeightTable& wt) {
    const fc_flow_config& c = f.cfg;
    Dims& d = f.d;
    if (c.struct_size != (int)sizeof(fc_flow_config)) throw Error(FC_ERR_INVALID, "fc_flow_config.struct_size mismatch (ABI)");
    if (c.latent_dim < c.input_dim) throw Error(FC_ERR_INVALID, "Latent dim < Input dim");
    if (c.cif_latent_dim < c.latent_dim) throw Error(FC_ERR_INVALID, "Augment dim smaller than main latent!");
    const bool cif = c.cif_latent_dim > c.latent_dim;
    if (cif && c.extra_context_dim) throw Error(FC_ERR_INVALID, "Not implemented extra context with cif");
    if (cif && c.global_context) throw Error(FC_ERR_INVALID, "CIF + global embedding not implemented");
    if (c.n_flow_layers < 1 || c.latent_dim < 2) throw Error(FC_ERR_INVALID, "need n_flow_layers >= 1 and latent_dim >= 2");
    if (c.extra_context_dim < 0 || c.extra_context_dim > 1) throw Error(FC_ERR_UNSUPPORTED, "extra_context_dim must be 0 or 1");
    d.Din = c.input_dim; d.D = c.latent_dim; d.d1 = d.D / 2; d.d2 = d.D - d.d1;
    d.d1_pad = round_up(d.d1, 32); d.d2_pad = round_up(d.d2, 32); d.ldx = d.d1_pad + d.d2_pad;
    d.E = c.input_embedding_dim; d.E_pad = round_up(d.E, 32); d.X = c.extra_context_dim;
    if (d.Din > 32) throw Error(FC_ERR_UNSUPPORTED, "input_dim > 32");
    d.Dc = c.cif_latent_dim; d.nz = d.Dc - d.D; d.nz_pad = round_up(std::max(d.nz, 1), 32);
    f.has_augment = d.D > d.Din;
    const int aug_slots = f.has_augment ? 1 : 0;
    std::vector<MatD> kv_rows(aug_slots + (c.global_context ? 0 : c.n_flow_layers));
    {
        std::vector<std::string> ap;
        if (f.has_augment) ap.push_back("transforms.0.attn");
        if (!c.global_context)
            for (int l = 0; l < c.n_flow_layers; ++l)
                ap.push_back("transforms." + std::to_string(1 + l * (2 + (c.act_norm ? 1 : 0))) + (cif ? ".flow" : "") + ".pre_conditioner.attn");
        f.kv_fold = kv_fold_gate(c, wt, ap);
    }
    std::mutex dims_mu;                          // d.H_pad / d.ldp maxima are the only shared writes of the per-layer builders

    // ---- transform 0: AugmentAttentionPreconditioner (models/augmenter.py:7-22) or IdentityTransform
    if (f.has_augment) {
        const std::string p = "transforms.0";
        build_precond(f, wt, p + ".attn", p + ".pre_attn_mlp", d.Din, 32, f.aug_pre, f.aug_attn, kv_rows, 0);
        const std::string pn = p + ".augment.noise_dist.net";
        pack_mlp_mid(f.arena, wt, pn, f.aug_net);
        f.aug_net.in_layer = build_in_layer(f, wt, pn, d.Din, 32, &f.aug_attn);
        build_pairs_out_layer(f, wt, pn, d.D - d.Din, f.aug_net);
        d.H_pad = std::max({d.H_pad, max_hidden_pad(f.aug_pre), max_hidden_pad(f.aug_net), d.A_in_pad});
    }
    // ---- blocks.  Layer l's transforms are [block, ActNorm?, permuter] at indices 1 + l * stride ...; the layers are independent, so
    //      after layer 0 (which fixes the shared attention dims) they are packed by a pool of host threads: the double-precision folds
    //      and the fp32 packing of 370 M weights (C2) are the bulk of fc_flow_create's time.
    f.blocks.resize(c.n_flow_layers);
    const int stride = 2 + (c.act_norm ? 1 : 0);
    auto build_block = [&](int l) {
        BlockPack& b = f.blocks[l];
        const int idx0 = 1 + l * stride;
        std::string p = "transforms." + std::to_string(idx0);
        b.has_attn = !c.global_context;
        b.has_cif = cif;
        int h_pad = 0, ldp = 0;
        if (cif) {
            build_cif(f, wt, p, b.cif);
            h_pad = std::max({h_pad, max_hidden_pad(b.cif.dist), max_hidden_pad(b.cif.aff)});
            p += ".flow";                              // the conditioned coupling lives one level down (cif_block.py:65)
        }
        if (b.has_attn) {
            build_precond(f, wt, p + ".pre_conditioner.attn", p + ".pre_conditioner.pre_attention_mlp", d.d1, d.d1_pad, b.pre, b.attn, kv_rows, aug_slots + l);
            h_pad = std::max({h_pad, max_hidden_pad(b.pre), d.A_in_pad});
        }
        const std::string pn = p + ".transform.nn";
        pack_mlp_mid(f.arena, wt, pn, b.net);
        b.net.in_layer = build_in_layer(f, wt, pn, d.d1, d.d1_pad, b.has_attn ? &b.attn : nullptr);
        build_out_layer(f, wt, pn, b.net);
        attach_mlp_rows_images(f.arena, b.net);
        h_pad = std::max(h_pad, max_hidden_pad(b.net));
        if (c.flow_type != FC_FLOW_AFFINE) ldp = b.net.out_layer.N_pad;
        if (c.flow_type == FC_FLOW_EXPONENTIAL) {
            if (d.d2 > kExpmWideMaxD2)   // the cap of include/fcflow.h (enum fc_flow_type): refused at create, not at the first forward
                throw Error(FC_ERR_UNSUPPORTED, "ExponentialCoupling: latent_dim - latent_dim/2 > 256 is not supported (the matrix-exponential action "
                                                "kernel holds at most a 256 x 256 matrix per point)");
            const std::string pt = p + ".transform";
            std::vector<float> sc = {wt.get(pt + ".scale", {1}).data[0], wt.get(pt + ".shift", {1}).data[0],
                                     wt.get(pt + ".rescale", {1}).data[0], wt.get(pt + ".reshift", {1}).data[0]};
            b.expm_scal = f.arena.upload(sc);
        }
        if (l != c.n_flow_layers - 1) build_lin(f, wt, c.act_norm ? idx0 + 1 : -1, idx0 + stride - 1, b);
        std::lock_guard<std::mutex> lock(dims_mu);
        d.H_pad = std::max(d.H_pad, h_pad);
        d.ldp = std::max(d.ldp, ldp);
    };
    build_block(0);
    {
        int dev = 0;
        FC_HIP(hipGetDevice(&dev));
        const int n_workers = std::max(1, std::min({(int)std::thread::hardware_concurrency(), 16, c.n_flow_layers - 1}));
        std::atomic<int> next{1};
        std::exception_ptr first_error;
        std::mutex err_mu;
        auto worker = [&]() {
            try {
                if (hipSetDevice(dev) != hipSuccess) throw Error(FC_ERR_HIP, "hipSetDevice failed in a packing thread");
                for (int l = next.fetch_add(1); l < c.n_flow_layers; l = next.fetch_add(1)) build_block(l);
            } catch (...) {
                std::lock_guard<std::mutex> lock(err_mu);
                if (!first_error) first_error = std::current_exception();
                next.store(c.n_flow_layers);
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < n_workers; ++t) pool.emplace_back(worker);
        worker();
        for (auto& t : pool) t.join();
        if (first_error) std::rethrow_exception(first_error);
    }
    for (const BlockPack& b : f.blocks) f.log_const += b.cif.log_const + b.log_const;      // fixed order: reproducible
    // ---- one stacked K|V projection for every attention
    f.n_attn = (int)kv_rows.size();
    if (f.n_attn && !f.kv_fold) {
        MatD all(f.n_attn * 2 * d.I_pad, d.E);
        for (int a = 0; a < f.n_attn; ++a) std::copy(kv_rows[a].v.begin(), kv_rows[a].v.end(), all.v.begin() + (size_t)a * 2 * d.I_pad * d.E);
        f.kv_all = pack_linear(f.arena, all, {}, {}, map_prefix(all.rows, all.rows), map_prefix(d.E, d.E_pad), {d.E_pad});
    }
}

// The inverse pass needs every folded ActNorm + permuter inverted (double precision): packed on the first fc_flow_inverse_f32, kept after
void ensure_lin_inverse(fc_flow& f) {
    const Dims& d = f.d;
    for (auto& b : f.blocks)
        if (b.has_lin && !b.has_lin_inv) {
            MatD inv = inverse_double(b.lin_w);
            VecD bi(d.D, 0.0);
            for (int i = 0; i < d.D; ++i) { double t = 0; for (int k = 0; k < d.D; ++k) t += inv.at(i, k) * b.lin_b[k]; bi[i] = -t; }
            const std::vector<int> xl = map_xlayout(d.d1, d.d1_pad, d.d2, d.d2_pad);
            b.lin_inv = pack_linear(f.arena, inv, bi, {}, xl, xl, {d.ldx});
            b.has_lin_inv = true;
        }
}

}  // namespace fc
