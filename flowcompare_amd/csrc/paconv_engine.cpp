// fc_paconv: the PAConv context embedder (PointNet++ SSG U-Net, models/scene_seg_PAConv/model/pointnet2/pointnet2_paconv_seg.py:14-82)
// as a launch schedule.  Per set-abstraction level l (n -> n/4 points, K = 32 neighbours, 3 PAConv layers):
//   fps -> gather new_xyz -> 32-NN (ascending) -> group + first-layer input E = [f - f_centre | f]
//   per layer: ScoreNet(xyz_nbr - xyz_centre) -> scores[edges, 8];  G = E @ weightbank  (fp32 MFMA GEMM, rows = edges, N = 8*Cout);
//              O = ReLU(BN(sum_m score_m G_m)) -> next E, or max over the 32 neighbours after the last layer.
// Per feature-propagation level: 3-NN inverse-distance interpolation + skip concat, then 1x1 conv + BN + ReLU as GEMMs
// with the BN folded into the weights.  Head: the shared head MLP (hostpack.h).
#include <algorithm>
#include <memory>

#include "hostpack.h"

namespace fc {
struct PaLayer {
    int cin = 0, cout = 0;      // PAConv input channels (before the x2 of kernel_input 'neighbor') and output channels
    PackedLinear bank;          // [8*cout][round32(2*cin)]
    float* score_w = nullptr;   // 200 floats, see scorenet_kernel
    float* bn_s = nullptr;
    float* bn_t = nullptr;
};
struct FpLayer { PackedLinear lin; int cout = 0; };
}  // namespace fc

struct fc_paconv {
    int* fp16_flag = nullptr;   // device word raised by the split-fp16 GEMM loop on an activation >= 65504 (common.h: Fp16Guard)
    fc::DeviceArena arena;
    int c_feat = 0;                       // input feature channels (input_dim - 3)
    std::vector<fc::PaLayer> sa[4];
    std::vector<fc::FpLayer> fp[4];
    int sa_out[4] = {0, 0, 0, 0};
    fc::HeadMLP head;
    static constexpr int K = 32;
};

namespace fc {

static void build_paconv(fc_paconv& e, const WeightTable& wt) {
    int prev = -1;
    for (int l = 0; l < 4; ++l) {
        for (int j = 0;; ++j) {
            const std::string p = "SA_modules." + std::to_string(l) + ".mlps.0.layer" + std::to_string(j);
            if (!wt.has(p + ".weightbank")) break;
            const HostTensor& wb = wt.get(p + ".weightbank");
            if (wb.shape.size() != 2 || wb.shape[0] % 2 || wb.shape[1] % 8) throw Error(FC_ERR_SHAPE, p + ".weightbank: expected [2*C_in, 8*C_out]");
            PaLayer L;
            L.cin = (int)wb.shape[0] / 2;
            L.cout = (int)wb.shape[1] / 8;
            if (j == 0) {
                if (l == 0) { e.c_feat = L.cin - 3; if (e.c_feat < 0 || e.c_feat > 29) throw Error(FC_ERR_UNSUPPORTED, "PAConv: input feature channels out of range"); }
                else if (L.cin != prev + 3) throw Error(FC_ERR_SHAPE, p + ".weightbank: C_in does not chain (+3 xyz)");
            } else if (L.cin != prev) throw Error(FC_ERR_SHAPE, p + ".weightbank: C_in does not chain");
            MatD bank = mat_from(wb);                              // [2cin][8cout] -> GEMM wants [N = 8cout][K = 2cin]
            MatD W(8 * L.cout, 2 * L.cin);
            for (int k = 0; k < 2 * L.cin; ++k) for (int n = 0; n < 8 * L.cout; ++n) W.at(n, k) = bank.at(k, n);
            L.bank = pack_linear(e.arena, W, {}, {}, map_prefix(8 * L.cout, 8 * L.cout), map_prefix(2 * L.cin, round_up(2 * L.cin, 32)),
                                 {round_up(2 * L.cin, 32)});
            // ScoreNet 3 -> 16 (no bias, BN, ReLU) -> 8 (bias); hidden [16], m = 8 (paconv.py:64-65 defaults)
            const HostTensor& w0 = wt.get(p + ".scorenet.mlp_convs_hidden.0.weight", {16, 3, 1, 1});
            const HostTensor& w1 = wt.get(p + ".scorenet.mlp_convs_hidden.1.weight", {8, 16, 1, 1});
            const HostTensor& b1 = wt.get(p + ".scorenet.mlp_convs_hidden.1.bias", {8});
            VecD s0, t0;
            bn_fold(wt, p + ".scorenet.mlp_bns_hidden.0", 16, s0, t0);
            std::vector<float> sw(200);
            for (int i = 0; i < 16; ++i) { for (int c = 0; c < 3; ++c) sw[3 * i + c] = (float)(s0[i] * w0.data[3 * i + c]); sw[48 + i] = (float)t0[i]; }
            for (int i = 0; i < 128; ++i) sw[64 + i] = w1.data[i];
            for (int i = 0; i < 8; ++i) sw[192 + i] = b1.data[i];
            L.score_w = e.arena.upload(sw);
            VecD s, t;
            bn_fold(wt, p + ".bn", L.cout, s, t);
            std::vector<float> fs(s.begin(), s.end()), ft(t.begin(), t.end());
            L.bn_s = e.arena.upload(fs);
            L.bn_t = e.arena.upload(ft);
            prev = L.cout;
            e.sa[l].push_back(L);
        }
        if (e.sa[l].empty()) throw Error(FC_ERR_MISSING, "SA_modules." + std::to_string(l) + ": no PAConv layers found");
        e.sa_out[l] = prev;
    }
    // feature propagation: FP_modules.i consumes level i (unknown, skip) and level i+1 (known)
    for (int i = 3; i >= 0; --i) {
        const int c_skip = i == 0 ? e.c_feat : e.sa_out[i - 1];
        int cin = -1;
        for (int j = 0;; ++j) {
            const std::string p = "FP_modules." + std::to_string(i) + ".mlp.layer" + std::to_string(j);
            if (!wt.has(p + ".conv.weight")) break;
            const HostTensor& w = wt.get(p + ".conv.weight");
            if (w.shape.size() != 4 || w.shape[2] != 1 || w.shape[3] != 1) throw Error(FC_ERR_SHAPE, p + ".conv.weight: expected 1x1 conv");
            const int co = (int)w.shape[0], ci = (int)w.shape[1];
            if (j == 0) {
                const int c_known = i == 3 ? e.sa_out[3] : e.fp[i + 1].back().cout;
                if (ci != c_known + c_skip) throw Error(FC_ERR_SHAPE, p + ".conv.weight: expected " + std::to_string(c_known + c_skip) + " input channels");
            } else if (ci != cin) throw Error(FC_ERR_SHAPE, p + ".conv.weight: channels do not chain");
            VecD s, t;
            bn_fold(wt, p + ".bn.bn", co, s, t);
            MatD W = mat_from(w);
            for (int o = 0; o < co; ++o) for (int c = 0; c < ci; ++c) W.at(o, c) *= s[o];
            FpLayer L;
            L.cout = co;
            L.lin = pack_linear(e.arena, W, t, {}, map_prefix(co, round_up(co, 32)), map_prefix(ci, round_up(ci, 32)), {round_up(ci, 32)});
            e.fp[i].push_back(L);
            cin = co;
        }
        if (e.fp[i].empty()) throw Error(FC_ERR_MISSING, "FP_modules." + std::to_string(i) + ": no layers found");
    }
    pack_head_mlp(e.arena, wt, "out_mlp", e.fp[0].back().cout, e.head);
}

struct PaWs {
    int n[5];                 // points per level
    float* xyz[5];            // [B*n_l][4]
    float* feat[5];           // level features, channels-last, pitch ldf[l]
    int ldf[5];
    int32_t *fidx, *nidx;
    float *gdiff, *scores, *Ea, *Eb, *G, *X, *Ya, *Yb, *h[3], *otmp, *fps_tmp;
    int P_pad;
};
static PaWs plan_pa(const fc_paconv& e, int B, int M, void* ws, size_t bytes, bool dry, size_t* need) {
    PaWs w{};
    WsCarver c(ws, bytes, dry);
    w.n[0] = M;
    for (int l = 1; l <= 4; ++l) w.n[l] = w.n[l - 1] / 4;
    for (int l = 0; l <= 4; ++l) {
        const int rows = round_up(std::max(B * w.n[l], 1), ROW_PAD);
        w.xyz[l] = c.floats((size_t)rows * 4);
        // features of a level: SA output first, later overwritten by the FP output (both <= 512 wide); level 0 holds the raw features
        const int width = round_up(std::max({l == 0 ? e.c_feat : e.sa_out[l - 1], l < 4 ? e.fp[l].back().cout : 0, 1}), 32);
        w.ldf[l] = width;
        w.feat[l] = c.floats((size_t)rows * width);
    }
    size_t emax = 1, gmax = 1, xmax = 1, edges_max = 1;
    for (int l = 0; l < 4; ++l) {
        const size_t edges = round_up(std::max(B * w.n[l + 1] * fc_paconv::K, 1), ROW_PAD);
        edges_max = std::max(edges_max, edges);
        for (const auto& L : e.sa[l]) {
            emax = std::max(emax, edges * (size_t)round_up(2 * L.cin, 32));
            gmax = std::max(gmax, edges * (size_t)(8 * L.cout));
        }
        const size_t rows = round_up(std::max(B * w.n[l], 1), ROW_PAD);
        for (const auto& L : e.fp[l]) xmax = std::max(xmax, rows * (size_t)std::max(L.lin.K_pad, L.lin.N_pad));
    }
    w.fidx = (int32_t*)c.bytes((size_t)B * std::max(w.n[1], 1) * sizeof(int32_t));
    w.nidx = (int32_t*)c.bytes(edges_max * sizeof(int32_t));
    w.fps_tmp = fps_scratch_floats(B, M) ? c.floats(fps_scratch_floats(B, M)) : nullptr;     // > 8192 points per scene: global min-distance array
    w.gdiff = c.floats(edges_max * 4);
    w.scores = c.floats(edges_max * 8);
    w.Ea = c.floats(emax);
    w.Eb = c.floats(emax);
    w.G = c.floats(gmax);
    w.X = c.floats(xmax);
    w.Ya = c.floats(xmax);
    w.Yb = c.floats(xmax);
    w.P_pad = round_up(B * M, ROW_PAD);
    for (int i = 0; i < 3; ++i) w.h[i] = c.floats((size_t)w.P_pad * e.head.H_pad);
    w.otmp = c.floats((size_t)w.P_pad * e.head.E_pad);
    if (need) *need = c.off + 256;
    return w;
}

// cnt: null for the uniform call.  With per-scene counts (fcflow_paconv_counts.h) scene b is embedded as its first count_b
// rows: level l of scene b stays at b * n[l] and uses its first count_b >> 2l rows.  The five kernels through which a row depends on its scene --
// FPS, the xyz gather, the 32-NN, the grouping, the 3-NN interpolation -- and score_reduce take the counts; ScoreNet, the GEMMs and the head run on
// the padded row count, whose pad rows are written as exact zeros wherever they enter a GEMM and in the output [B, M, E].
static void paconv_forward(fc_paconv& e, const char* who, const float* pts, const SceneCounts* cnt, float* out, int B, int M, void* ws, size_t bytes, hipStream_t s) {
    if (!pts || !out || B < 1) throw Error(FC_ERR_INVALID, std::string(who) + ": bad argument");
    if (cnt && !cnt->counts) throw Error(FC_ERR_INVALID, std::string(who) + ": null counts (the call without counts is fc_paconv_embed_f32)");
    if ((cnt ? std::min(cnt->lo, M) : M) < 256) throw Error(FC_ERR_INVALID, "PAConv embedder needs at least 256 context points (four 4x farthest-point down-samplings)");
    if (cnt && (cnt->lo > cnt->hi || cnt->hi > M)) throw Error(FC_ERR_INVALID, std::string(who) + ": counts must satisfy 256 <= count_min <= count_max <= M");
    constexpr int K = fc_paconv::K;
    PaWs w = plan_pa(e, B, M, ws, bytes, false, nullptr);
    const int ldp = 3 + e.c_feat;
    auto lvl = [&](int l) { return LevelCounts{cnt->counts, cnt->lo, cnt->hi, 2 * l}; };      // the scene's rows at level l: count_b >> 2l
    // level 0: xyz (pitch 4) and raw features (pitch 32)
    launch_fill(w.xyz[0], 0.f, (size_t)round_up(B * M, ROW_PAD) * 4, s);
    launch_pack_rows(pts, ldp, 3, w.xyz[0], 4, 0, 4, B * M, s);
    launch_fill(w.feat[0], 0.f, (size_t)round_up(B * M, ROW_PAD) * w.ldf[0], s);
    if (e.c_feat > 0) launch_pack_rows(pts + 3, ldp, e.c_feat, w.feat[0], w.ldf[0], 0, e.c_feat, B * M, s);
    if (cnt) {                                             // (a NaN or 1e30 in the caller's pad rows stays out of every panel)
        launch_zero_pad_rows(w.xyz[0], 4, cnt->counts, B, M, s);
        launch_zero_pad_rows(w.feat[0], w.ldf[0], cnt->counts, B, M, s);
    }
    int cprev = e.c_feat;
    // ---- set abstraction
    for (int l = 0; l < 4; ++l) {
        const int n = w.n[l], m = w.n[l + 1], edges = B * m * K, edges_pad = round_up(std::max(edges, 1), ROW_PAD);
        float* Ein = w.Ea;
        float* Eout = w.Eb;
        const int ldE0 = e.sa[l][0].bank.K_pad;
        if (cnt) {
            launch_fps_counts(w.xyz[l], 4, w.fidx, B, n, m, w.fps_tmp, lvl(l), s);
            launch_gather_xyz_counts(w.xyz[l], 4, w.fidx, w.xyz[l + 1], B, n, m, lvl(l + 1), s);
            launch_knn_xyz_counts(w.xyz[l], 4, w.xyz[l + 1], w.nidx, B, n, m, K, lvl(l), lvl(l + 1), s);
            launch_paconv_group_counts(w.xyz[l], 4, w.feat[l], w.ldf[l], cprev, w.xyz[l + 1], w.nidx, Ein, ldE0, w.gdiff, B, n, m, K, lvl(l + 1), s);
        } else {
            launch_fps(w.xyz[l], 4, w.fidx, B, n, m, w.fps_tmp, s);
            launch_gather_xyz(w.xyz[l], 4, w.fidx, w.xyz[l + 1], B, n, m, s);
            launch_knn_xyz(w.xyz[l], 4, w.xyz[l + 1], w.nidx, B, n, m, K, s);
            launch_paconv_group(w.xyz[l], 4, w.feat[l], w.ldf[l], cprev, w.xyz[l + 1], w.nidx, Ein, ldE0, w.gdiff, B, n, m, K, s);
        }
        for (size_t j = 0; j < e.sa[l].size(); ++j) {
            const PaLayer& L = e.sa[l][j];
            launch_scorenet(w.gdiff, L.score_w, w.scores, edges, s);
            GemmEpi g{};
            g.C = w.G; g.ldc = 8 * L.cout; g.rows_valid = edges;
            ASeg a{Ein, L.bank.K_pad};
            launch_gemm(L.bank, &a, edges_pad, g, EPI_LINEAR, s);
            const bool last = j + 1 == e.sa[l].size();
            if (!last) {
                if (cnt) launch_score_reduce_counts(w.G, 8 * L.cout, w.scores, L.bn_s, L.bn_t, L.cout, K, Eout, e.sa[l][j + 1].bank.K_pad, 0, 0, B, m, lvl(l + 1), s);
                else launch_score_reduce(w.G, 8 * L.cout, w.scores, L.bn_s, L.bn_t, L.cout, K, Eout, e.sa[l][j + 1].bank.K_pad, 0, 0, B * m, s);
                std::swap(Ein, Eout);
            } else {
                launch_fill(w.feat[l + 1], 0.f, (size_t)round_up(std::max(B * m, 1), ROW_PAD) * w.ldf[l + 1], s);
                if (cnt) launch_score_reduce_counts(w.G, 8 * L.cout, w.scores, L.bn_s, L.bn_t, L.cout, K, w.feat[l + 1], w.ldf[l + 1], 0, 1, B, m, lvl(l + 1), s);
                else launch_score_reduce(w.G, 8 * L.cout, w.scores, L.bn_s, L.bn_t, L.cout, K, w.feat[l + 1], w.ldf[l + 1], 0, 1, B * m, s);
            }
        }
        cprev = e.sa_out[l];
    }
    // ---- feature propagation (level 3 <- 4, 2 <- 3, 1 <- 2, 0 <- 1); a level's features are replaced by the FP output
    int c_known = e.sa_out[3];
    for (int i = 3; i >= 0; --i) {
        const int nu = w.n[i], mk = w.n[i + 1], rows = B * nu, rows_pad = round_up(std::max(rows, 1), ROW_PAD);
        const int c_skip = i == 0 ? e.c_feat : e.sa_out[i - 1];
        const int ldX = e.fp[i][0].lin.K_pad;
        if (cnt) launch_three_nn_interp_counts(w.xyz[i], 4, w.xyz[i + 1], 4, w.feat[i + 1], w.ldf[i + 1], c_known, w.feat[i], w.ldf[i], c_skip, w.X, ldX, B, nu, mk, lvl(i), lvl(i + 1), s);
        else launch_three_nn_interp(w.xyz[i], 4, w.xyz[i + 1], 4, w.feat[i + 1], w.ldf[i + 1], c_known, w.feat[i], w.ldf[i], c_skip, w.X, ldX, B, nu, mk, s);
        const float* cur = w.X;
        int ldcur = ldX;
        for (size_t j = 0; j < e.fp[i].size(); ++j) {
            const FpLayer& L = e.fp[i][j];
            const bool last = j + 1 == e.fp[i].size();
            float* dst = last ? w.feat[i] : (cur == w.Ya ? w.Yb : w.Ya);
            const int ldd = last ? w.ldf[i] : L.lin.N_pad;
            if (last && w.ldf[i] < L.lin.N_pad) throw Error(FC_ERR_INVALID, "PAConv: level feature pitch too small");
            GemmEpi g{};
            g.C = dst; g.ldc = ldd; g.act = FC_ACT_RELU; g.rows_valid = rows;
            ASeg a{cur, ldcur};
            launch_gemm(L.lin, &a, rows_pad, g, EPI_LINEAR, s);
            cur = dst;
            ldcur = ldd;
        }
        c_known = e.fp[i].back().cout;
    }
    // ---- head MLP on level 0
    run_head_mlp(e.head, {w.feat[0], w.ldf[0]}, w.h, w.otmp, out, B * M, w.P_pad, B * M, s);
    if (cnt) launch_zero_tail_rows(out, e.head.E, B, M, *cnt, s);        // (the head ran on the pad rows too: [B, M, E] gets 0.0f there)
}

}  // namespace fc


extern "C" {

int fc_paconv_create(const fc_tensor* tensors, int32_t n_tensors, fc_paconv** out) {
    FC_API_BEGIN
    if (!out) throw fc::Error(FC_ERR_INVALID, "fc_paconv_create: null out");
    *out = nullptr;
    std::unique_ptr<fc_paconv> e(new fc_paconv());
    fc::WeightTable wt(tensors, n_tensors);
    fc::build_paconv(*e, wt);
    *out = fc::finish_create(e);
    FC_API_END
}
void fc_paconv_destroy(fc_paconv* emb) { delete emb; }
int fc_paconv_out_dim(const fc_paconv* emb) { return emb ? emb->head.E : 0; }
int fc_paconv_workspace_bytes(const fc_paconv* emb, int32_t B, int32_t M, size_t* bytes) {
    FC_API_BEGIN
    if (!emb || !bytes || B < 1 || M < 1) throw fc::Error(FC_ERR_INVALID, "fc_paconv_workspace_bytes: bad argument");
    fc::plan_pa(*emb, B, M, nullptr, 0, true, bytes);
    FC_API_END
}
int fc_paconv_embed_f32(fc_paconv* emb, const float* pts, float* out, int32_t B, int32_t M, void* workspace, size_t workspace_bytes, void* stream) {
    FC_API_BEGIN
    fc::embed_guarded(emb, workspace, "fc_paconv_embed_f32", (hipStream_t)stream, [=] {
        fc::paconv_forward(*emb, "fc_paconv_embed_f32", pts, nullptr, out, B, M, workspace, workspace_bytes, (hipStream_t)stream);
    });
    FC_API_END
}
/* declared in fcflow_paconv_counts.h */
int fc_paconv_embed_counts_f32(fc_paconv* emb, const float* pts, const int32_t* counts, int32_t count_min, int32_t count_max, float* out, int32_t B, int32_t M,
                               void* workspace, size_t workspace_bytes, void* stream) {
    FC_API_BEGIN
    const fc::SceneCounts cnt{counts, count_min, count_max};
    fc::embed_guarded(emb, workspace, "fc_paconv_embed_counts_f32", (hipStream_t)stream, [=] {
        fc::paconv_forward(*emb, "fc_paconv_embed_counts_f32", pts, &cnt, out, B, M, workspace, workspace_bytes, (hipStream_t)stream);
    });
    FC_API_END
}
/* the engine's counted FPS launch on its own: xyz [B, n, 3], idx [B, m] with m = n >> 2 */
int fc_op_fps_counts_f32(const float* xyz, const int32_t* counts, int32_t count_min, int32_t count_max, int32_t* idx, int32_t B, int32_t n, int32_t m, void* stream) {
    FC_API_BEGIN
    if (!xyz || !counts || !idx) throw fc::Error(FC_ERR_INVALID, "fc_op_fps_counts_f32: null pointer");
    if (B < 1 || n < 4 || m != n >> 2) throw fc::Error(FC_ERR_INVALID, "fc_op_fps_counts_f32: bad argument (m must be n >> 2, n >= 4)");
    if (count_min < 4 || count_min > count_max || count_max > n) throw fc::Error(FC_ERR_INVALID, "fc_op_fps_counts_f32: counts must satisfy 4 <= count_min <= count_max <= n");
    float* scratch = nullptr;
    const size_t nf = fc::fps_scratch_floats(B, n);
    if (nf) FC_HIP(hipMallocAsync((void**)&scratch, nf * sizeof(float), (hipStream_t)stream));
    try { fc::launch_fps_counts(xyz, 3, idx, B, n, m, scratch, fc::LevelCounts{counts, count_min, count_max, 0}, (hipStream_t)stream); }
    catch (...) { if (scratch) (void)hipFreeAsync(scratch, (hipStream_t)stream); throw; }
    if (scratch) FC_HIP(hipFreeAsync(scratch, (hipStream_t)stream));
    FC_API_END
}
/* the engine's counted 32-NN launch on its own: xyz [B, n, 4], qxyz [B, m, 4], out [B, m, k]; counts_n in [1, n], counts_m in [0, m] (clamped) */
int fc_op_paconv_knn_counts_f32(const float* xyz, const float* qxyz, const int32_t* counts_n, const int32_t* counts_m, int32_t* out, int32_t B, int32_t n, int32_t m,
                                int32_t k, void* stream) {
    FC_API_BEGIN
    if (!xyz || !qxyz || !counts_n || !counts_m || !out) throw fc::Error(FC_ERR_INVALID, "fc_op_paconv_knn_counts_f32: null pointer");
    if (B < 1 || n < 1 || m < 1 || k < 1) throw fc::Error(FC_ERR_INVALID, "fc_op_paconv_knn_counts_f32: bad argument");
    fc::launch_knn_xyz_counts(xyz, 4, qxyz, out, B, n, m, k, fc::LevelCounts{counts_n, 1, n, 0}, fc::LevelCounts{counts_m, 0, m, 0}, (hipStream_t)stream);
    FC_API_END
}

}  // extern "C"
