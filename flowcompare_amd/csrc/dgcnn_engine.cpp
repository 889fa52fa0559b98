// fc_dgcnn: DGCNN context embedder (models/pytorch_gcn.py:50-188), eval mode, as a launch schedule.
//
// Per edge-conv level (C_in -> C_out, k neighbours):
//   reference:  knn -> gather -> cat(nbr - x, x) [B,2C,M,k] -> 1x1 conv -> BN2d -> LeakyReLU(0.2) -> max_k
//   here:       knn (fused distance + streaming top-k, no MxM matrix)
//               one GEMM  uv = f [W1' ; W2'-W1']^T + [0 ; t]      (conv is linear: W (nbr - x | x) = W1 nbr + (W2 - W1) x;
//                                                                  eval BN = per-channel scale s / shift t, s folded into both halves)
//               gather-max: out = LeakyReLU( max_j u[idx_j] + v )  (LeakyReLU is increasing, so it commutes with max)
//   which does k x fewer conv FLOPs and never builds the [B,2C,M,k] edge tensor.
// conv5 + BN1d fold into one GEMM with a LeakyReLU epilogue; out_mlp is the shared head MLP (hostpack.h).
#include <algorithm>
#include <memory>

#include "hostpack.h"

struct fc_dgcnn {
    int* fp16_flag = nullptr;   // device word raised by the split-fp16 GEMM loop on an activation >= 65504 (common.h: Fp16Guard)
    fc::DeviceArena arena;
    int k = 0, global_pool = 0, c_in = 0;
    fc::PackedLinear level[4];
    int lvl_cin[4] = {0, 0, 0, 0}, lvl_cout[4] = {64, 64, 128, 256}, lvl_col[4] = {0, 64, 128, 256};
    fc::PackedLinear conv5;
    fc::HeadMLP head;
};

namespace fc {

static void build_dgcnn(fc_dgcnn& e, const WeightTable& wt) {
    int cin = -1;
    for (int l = 0; l < 4; ++l) {
        const std::string p = "conv" + std::to_string(l + 1);
        const HostTensor& w = wt.get(p + ".0.weight");
        const int co = e.lvl_cout[l];
        if (w.shape.size() != 4 || w.shape[0] != co || w.shape[2] != 1 || w.shape[3] != 1 || w.shape[1] % 2)
            throw Error(FC_ERR_SHAPE, p + ".0.weight: expected [C_out, 2*C_in, 1, 1]");
        const int ci = (int)w.shape[1] / 2;
        if (l == 0) { cin = ci; e.c_in = ci; if (ci > 32) throw Error(FC_ERR_UNSUPPORTED, "DGCNN input_dim > 32"); }
        else if (ci != e.lvl_cout[l - 1]) throw Error(FC_ERR_SHAPE, p + ".0.weight: C_in does not chain");
        e.lvl_cin[l] = ci;
        VecD s, t;
        bn_fold(wt, p + ".1", co, s, t);
        MatD W = mat_from(w);                       // [co][2ci] : first ci columns act on (nbr - x), last ci on x
        MatD F(2 * co, ci);
        VecD b(2 * co, 0.0);
        for (int o = 0; o < co; ++o) {
            for (int c = 0; c < ci; ++c) {
                F.at(o, c) = s[o] * W.at(o, c);
                F.at(co + o, c) = s[o] * (W.at(o, ci + c) - W.at(o, c));
            }
            b[co + o] = t[o];
        }
        e.level[l] = pack_linear(e.arena, F, b, {}, map_prefix(2 * co, 2 * co), map_prefix(ci, round_up(ci, 32)), {round_up(ci, 32)});
    }
    (void)cin;
    {
        const HostTensor& w = wt.get("conv5.0.weight", {512, 512, 1});
        VecD s, t;
        bn_fold(wt, "conv5.1", 512, s, t);
        MatD W = mat_from(w);
        for (int o = 0; o < 512; ++o) for (int c = 0; c < 512; ++c) W.at(o, c) *= s[o];
        e.conv5 = pack_linear(e.arena, W, t, {}, map_prefix(512, 512), map_prefix(512, 512), {512});
    }
    pack_head_mlp(e.arena, wt, "out_mlp", e.global_pool ? 1024 : 512, e.head);
}

struct DgWs {
    float *pts, *cat, *uv, *t5, *h[3], *pool, *otmp;
    int32_t* idx;
    int P, P_pad, R_pad;     // R = rows of the MLP stage (P per-point, B global)
};
static DgWs plan_dg(const fc_dgcnn& e, int B, int M, void* ws, size_t bytes, bool dry, size_t* need) {
    DgWs w{};
    w.P = B * M; w.P_pad = round_up(w.P, ROW_PAD);
    w.R_pad = e.global_pool ? round_up(B, ROW_PAD) : w.P_pad;
    WsCarver c(ws, bytes, dry);
    w.pts = c.floats((size_t)w.P_pad * 32);
    w.cat = c.floats((size_t)w.P_pad * 512);
    w.uv = c.floats((size_t)w.P_pad * 512);
    w.t5 = c.floats((size_t)w.P_pad * 512);
    w.idx = (int32_t*)c.bytes((size_t)w.P * e.k * sizeof(int32_t));
    for (int i = 0; i < 3; ++i) w.h[i] = c.floats((size_t)w.R_pad * e.head.H_pad);
    w.pool = c.floats(e.global_pool ? (size_t)w.R_pad * 1024 : 1);
    w.otmp = c.floats((size_t)w.R_pad * e.head.E_pad);
    if (need) *need = c.off + 256;
    return w;
}

// cnt: null for the uniform call.  With per-scene counts (fcflow_embed_counts.h) scene b is embedded as its first M_b rows: the three places
// where a row depends on its scene -- the k-NN search, the gather-max behind it, the global pool -- take the count, everything else is
// row-wise GEMM on the padded batch, whose pad rows are kept at exact zeros going in (w.pts, the cat panel) and coming out ([B, M, E]).
static void dgcnn_forward(fc_dgcnn& e, const char* who, const float* pts, const SceneCounts* cnt, float* out, int B, int M, void* ws, size_t bytes, hipStream_t s) {
    if (!pts || !out || B < 1 || M < 1) throw Error(FC_ERR_INVALID, std::string(who) + ": bad argument");
    if (cnt && !cnt->counts) throw Error(FC_ERR_INVALID, std::string(who) + ": null counts (the call without counts is fc_dgcnn_embed_f32)");
    if ((cnt ? cnt->lo : M) < e.k) throw Error(FC_ERR_INVALID, "fewer context points than n_neighbors (torch.topk raises in the reference)");
    if (cnt && (cnt->lo > cnt->hi || cnt->hi > M)) throw Error(FC_ERR_INVALID, std::string(who) + ": counts must satisfy n_neighbors <= count_min <= count_max <= M");
    DgWs w = plan_dg(e, B, M, ws, bytes, false, nullptr);
    launch_fill(w.pts, 0.f, (size_t)w.P_pad * 32, s);
    launch_pack_rows(pts, e.c_in, e.c_in, w.pts, 32, 0, 32, w.P, s);
    if (cnt) launch_zero_pad_rows(w.pts, 32, cnt->counts, B, M, s);      // (a NaN or 1e30 in the caller's pad rows reaches neither the range flag nor a GEMM)
    if (w.P_pad > w.P) launch_fill(w.cat + (size_t)w.P * 512, 0.f, (size_t)(w.P_pad - w.P) * 512, s);
    for (int l = 0; l < 4; ++l) {
        const float* f = l == 0 ? w.pts : w.cat + e.lvl_col[l - 1];
        const int ldf = l == 0 ? 32 : 512;
        // (levels 1-3: warm start from the previous level's sets, in place)
        if (cnt) launch_knn_counts(f, ldf, e.lvl_cin[l], w.idx, B, M, M, e.k, s, l > 0 ? w.idx : nullptr, *cnt);
        else launch_knn(f, ldf, e.lvl_cin[l], w.idx, B, M, M, e.k, s, l > 0 ? w.idx : nullptr);
        GemmEpi g{};
        g.C = w.uv; g.ldc = 512;
        ASeg a{f, ldf};
        launch_gemm(e.level[l], &a, w.P_pad, g, EPI_LINEAR, s);
        if (cnt) launch_gather_max_counts(w.uv, 512, e.lvl_cout[l], w.idx, e.k, w.cat, 512, e.lvl_col[l], B, M, M, *cnt, s);
        else launch_gather_max(w.uv, 512, e.lvl_cout[l], w.idx, e.k, w.cat, 512, e.lvl_col[l], B, M, M, s);
    }
    {
        GemmEpi g{};
        g.C = w.t5; g.ldc = 512; g.act = FC_ACT_LRELU02;
        ASeg a{w.cat, 512};
        launch_gemm(e.conv5, &a, w.P_pad, g, EPI_LINEAR, s);
    }
    ASeg in{w.t5, 512};
    int rows = w.P, rows_pad = w.P_pad;
    if (e.global_pool) {
        launch_fill(w.pool, 0.f, (size_t)w.R_pad * 1024, s);
        if (cnt) launch_pool_max_mean_counts(w.t5, 512, 512, w.pool, 1024, B, M, M, *cnt, s);
        else launch_pool_max_mean(w.t5, 512, 512, w.pool, 1024, B, M, M, s);
        in = {w.pool, 1024};
        rows = B; rows_pad = w.R_pad;
    }
    run_head_mlp(e.head, in, w.h, w.otmp, out, rows, rows_pad, 0, s);       // (the out_layer launch of this engine sets no rows_valid)
    if (cnt && !e.global_pool) launch_zero_tail_rows(out, e.head.E, B, M, *cnt, s);   // (the head ran on the pad rows too: [B, M, E] gets 0.0f there)
}

const char* get_last_error();
}  // namespace fc


extern "C" {

int fc_dgcnn_create(int32_t n_neighbors, int32_t global_pool, const fc_tensor* tensors, int32_t n_tensors, fc_dgcnn** out) {
    FC_API_BEGIN
    if (!out) throw fc::Error(FC_ERR_INVALID, "fc_dgcnn_create: null out");
    *out = nullptr;
    if (n_neighbors < 1 || n_neighbors > 64) throw fc::Error(FC_ERR_UNSUPPORTED, "n_neighbors must be in [1, 64]");
    std::unique_ptr<fc_dgcnn> e(new fc_dgcnn());
    e->k = n_neighbors;
    e->global_pool = global_pool ? 1 : 0;
    fc::WeightTable wt(tensors, n_tensors);
    fc::build_dgcnn(*e, wt);
    *out = fc::finish_create(e);
    FC_API_END
}
void fc_dgcnn_destroy(fc_dgcnn* emb) { delete emb; }
int fc_dgcnn_out_dim(const fc_dgcnn* emb) { return emb ? emb->head.E : 0; }
int fc_dgcnn_workspace_bytes(const fc_dgcnn* emb, int32_t B, int32_t M, size_t* bytes) {
    FC_API_BEGIN
    if (!emb || !bytes || B < 1 || M < 1) throw fc::Error(FC_ERR_INVALID, "fc_dgcnn_workspace_bytes: bad argument");
    fc::plan_dg(*emb, B, M, nullptr, 0, true, bytes);
    FC_API_END
}
int fc_dgcnn_embed_f32(fc_dgcnn* emb, const float* pts, float* out, int32_t B, int32_t M, void* workspace, size_t workspace_bytes, void* stream) {
    FC_API_BEGIN
    fc::embed_guarded(emb, workspace, "fc_dgcnn_embed_f32", (hipStream_t)stream, [=] {
        fc::dgcnn_forward(*emb, "fc_dgcnn_embed_f32", pts, nullptr, out, B, M, workspace, workspace_bytes, (hipStream_t)stream);
    });
    FC_API_END
}
/* declared in fcflow_embed_counts.h */
int fc_dgcnn_embed_counts_f32(fc_dgcnn* emb, const float* pts, const int32_t* counts, int32_t count_min, int32_t count_max, float* out, int32_t B, int32_t M,
                              void* workspace, size_t workspace_bytes, void* stream) {
    FC_API_BEGIN
    const fc::SceneCounts cnt{counts, count_min, count_max};
    fc::embed_guarded(emb, workspace, "fc_dgcnn_embed_counts_f32", (hipStream_t)stream, [=] {
        fc::dgcnn_forward(*emb, "fc_dgcnn_embed_counts_f32", pts, &cnt, out, B, M, workspace, workspace_bytes, (hipStream_t)stream);
    });
    FC_API_END
}

}  // extern "C"
