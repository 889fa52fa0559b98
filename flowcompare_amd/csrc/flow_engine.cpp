// fc_flow, the per-call half: the conditional normalizing flow (augmenter -> n x [pre-conditioner -> coupling -> ActNorm -> permuter]
// -> base density) as a schedule of HIP kernel launches over a caller-owned workspace, and the fc_flow_* entry points.  The packed model it
// reads is built once by flow_pack.cpp (flow_model.h).
// Activation layout in HBM: x is [rows, d1_pad + d2_pad] = [x1 | 0-pad | x2 | 0-pad] (pads kept zero by construction), every
// other activation is [rows, round_up(width, 32)]; rows are padded to 256.
#include <algorithm>
#include <cstring>
#include <memory>

#include "flow_model.h"

namespace fc {

// ---------------------------------------------------------------- workspace plan
struct FlowWs {
    float *xa, *xb, *h[3], *q, *a, *ctxp, *kv, *xin, *rowscal, *spl, *cbuf;
    void* kv16;      // K / V limb images of the layer in flight (split-fp16 attention); with the K|V fold: the context panel's one image
    const unsigned short* ctx16;   // K|V fold, split-fp16 attention: kv16 holds the context limb image of this forward (prepare); else null
    float* ldjp;     // log-det partial slots of the fused spline / pair epilogues, [ldj_slots][P_pad] (ldj_slot_count)
    int ldj_slots;
    bool kv_limbs;         // w.kv holds the K|V projections as the GEMM's fp16 limb image (GemmEpi::C16) instead of fp32
    float* lnss;           // [A_in / 64][P_pad] per-row sums of squares of the centred pre-MLP output (LayerNorm -> q fold)
    unsigned short* h16;   // fp16 limb image of the last hidden activation feeding the spline parameter GEMM (limb chain)
    int P, P_pad, Pc, Pc_pad, ldkv;
    int spl_rows;          // rows of w.spl: P_pad, or the row chunk of the wide ExponentialCoupling (expm_chunk_rows)
    float* lp_scratch;     // [P_pad] log-prob accumulator of a pass whose caller wants none (fc_flow_attention_weights_f32 with logprob = NULL)
    const int32_t* m_counts;   // per-scene context point counts of this call (device [B], fcflow_context_counts.h) or null: every attention's AttnProblem
    void ldj_into(GemmEpi& e) const { e.ldj_part = ldjp; e.ldj_pitch = (size_t)P_pad; }      // the epilogue accumulates its log-det partials in ldjp
};
// Log-det partial slots (rows of FlowWs::ldjp): one per 128-column tile of the fused spline epilogue, two (one per wave column)
// per 128-column tile of a pair-packed epilogue (affine coupling, augmenter, CIF slice) on the 8-wave split-fp16 tile.  The
// epilogues ACCUMULATE into their own slots over the layers; flow_forward zeroes the buffer first and reduces it once at the end,
// in a fixed order (bit-reproducible, unlike atomics on log-prob).
static int ldj_slot_count(const fc_flow& f) {
    int n = f.cfg.flow_type == FC_FLOW_SPLINE ? f.d.ldp / 128 : 0;
    auto pair = [&](const PackedLinear& L) { if (L.N_pad > 0) n = std::max(n, 2 * (round_up(L.N_pad, 128) / 128)); };
    if (f.has_augment) pair(f.aug_net.out_layer);
    for (const BlockPack& b : f.blocks) {
        if (f.cfg.flow_type == FC_FLOW_AFFINE) pair(b.net.out_layer);
        if (b.has_cif) { pair(b.cif.dist.out_layer); pair(b.cif.aff.out_layer); }
    }
    return n;
}

// ExponentialCoupling with d2 > 16 emits d2^2 + d2 parameters per point (90.6 KB at d2 = 150): the out-layer GEMM and the expm kernel run
// chunk by chunk over row blocks whose parameter panel stays within kExpmChunkBytes (2048 rows at d2 = 150), so the panel does not grow with
// B x N and a chunk's panel can be read back from the 256 MiB Infinity Cache.
constexpr size_t kExpmChunkBytes = 192ull << 20;
static int expm_chunk_rows(const fc_flow& f, int P_pad) {
    const size_t per = (size_t)f.d.ldp * sizeof(float);
    const int c = std::max(ROW_PAD, (int)(kExpmChunkBytes / per) / ROW_PAD * ROW_PAD);
    return std::min(c, P_pad);
}

static FlowWs plan_ws(const fc_flow& f, int B, int N, int M, void* ws, size_t bytes, bool dry, size_t* need) {
    const Dims& d = f.d;
    FlowWs w{};
    w.P = B * N; w.P_pad = round_up(w.P, ROW_PAD);
    w.Pc = B * M; w.Pc_pad = round_up(w.Pc, ROW_PAD);
    w.ldkv = f.kv_fold ? 0 : f.n_attn * 2 * d.I_pad;      // (K|V fold: no projected K|V, no region for them)
    WsCarver c(ws, bytes, dry);
    w.xa = c.floats((size_t)w.P_pad * d.ldx);
    w.xb = c.floats((size_t)w.P_pad * d.ldx);
    for (int i = 0; i < 3; ++i) w.h[i] = c.floats((size_t)w.P_pad * d.ldh());
    w.q = c.floats((size_t)w.P_pad * std::max(d.I_pad, 32));
    w.a = c.floats((size_t)w.P_pad * std::max(d.I_pad, 32));
    w.ctxp = c.floats((size_t)w.Pc_pad * d.E_pad);
    w.kv = f.kv_fold ? nullptr : c.floats((size_t)w.Pc_pad * std::max(w.ldkv, 32));
    w.xin = c.floats((size_t)w.P_pad * 32);
    w.rowscal = c.floats((size_t)w.P_pad);
    w.spl_rows = expm_wide(f) ? expm_chunk_rows(f, w.P_pad) : w.P_pad;
    w.spl = c.floats(d.ldp ? (size_t)w.spl_rows * d.ldp : 1);
    w.cbuf = c.floats(d.nz > 0 ? (size_t)w.P_pad * d.nz_pad : 1);
    w.ldj_slots = ldj_slot_count(f);
    w.ldjp = c.floats(std::max<size_t>((size_t)w.ldj_slots * w.P_pad, 1));
    w.h16 = (unsigned short*)c.bytes((size_t)w.P_pad * d.ldh() * 4);
    w.lnss = c.floats(f.n_attn > 0 ? (size_t)(std::max(d.A_in, 64) / 64) * w.P_pad : 1);
    w.kv16 = c.bytes(f.n_attn > 0 ? std::max<size_t>(attention_limb_ws_bytes(w.Pc_pad, d.I_pad) / (f.kv_fold ? 2 : 1), 16) : 16);
    w.lp_scratch = c.floats((size_t)w.P_pad);
    if (need) *need = c.off + 256;
    return w;
}

// Diagnostic (fc_debug_flow_trace, ops_api.cpp; tests/fullsize_util.py): when the calling thread has set a buffer, flow_forward copies the
// x2 half of the latent AS THE COUPLING OF LAYER l WILL READ IT into trace[l][row][d2] -- the fp32 values the spline's inside / outside
// decision |x2| <= 3 is taken on (models/spline_coupling.py:35-48), so a test can hand the fp64 oracle the HIP run's own decisions.
thread_local float* t_flow_trace = nullptr;
thread_local size_t t_flow_trace_floats = 0;
void flow_set_trace(float* buf, size_t floats) { t_flow_trace = buf; t_flow_trace_floats = floats; }
thread_local float* t_expm_info = nullptr;      // fc_debug_expm_info: per-point statistics of the wide ExponentialCoupling kernel
thread_local size_t t_expm_info_floats = 0;
void flow_set_expm_info(float* buf, size_t floats) { t_expm_info = buf; t_expm_info_floats = floats; }

// the plain EPI_LINEAR epilogue: C[rows_valid][ldc] = A W^T + bias, nothing else
static GemmEpi linear_epi(float* C, int ldc, int rows_valid) {
    GemmEpi e{};
    e.C = C; e.ldc = ldc; e.rows_valid = rows_valid;
    return e;
}
// Limb chain: `producer` writes its output once as the fp16 limb image (GemmEpi::C16) and `consumer` copies it (A16) instead of re-splitting
// the fp32 rows per column tile.  The shapes both ends need; every site adds the widths its own kernels take.
static bool limb_chain_pair(const PackedLinear& producer, const PackedLinear& consumer) {
    return producer.W2 != nullptr && consumer.W2 != nullptr && producer.N_pad == consumer.K_pad && consumer.nseg == 1;
}

static int run_mlp_hidden(const fc_flow& f, const PackedMLP& m, const ASeg* in_segs, const float* rowscal, FlowWs& w, int act, hipStream_t s,
                          unsigned short* last_limbs = nullptr, float last_scale = 0.f) {
    // 512-wide coupling nets inside a guard scope: in_layer + hidden layers as ONE row-resident launch (mlprows.hip); the scratch images
    // of its intermediate activations live in the h[] buffers (same 2 KB per row as a 512-wide fp32 panel)
    // (a workgroup owns 128 rows for the whole chain: with fewer workgroups than ~3/4 of the CUs -- C1's 2 x 1024 points are 16 -- the chain
    // of ONE workgroup is the launch's duration and the per-layer launches on 64 x 64 tiles are faster: 21 vs 38 ms per C1 step)
    if (last_limbs && f.d.H_pad == 512 && gemm_limb_chain_all_ok() && mlp_rows_eligible(m.in_layer, m.mid, act) && mlp_rows_fills_the_chip(w.P_pad)) {
        launch_mlp_rows(m.in_layer, m.mid, in_segs, rowscal, act, w.h, last_limbs, w.P_pad, w.P, s, last_scale);
        return -1;
    }
    return run_mlp_hidden_generic(m, in_segs, rowscal, act, w.h, f.d.ldh(), w.P_pad, s, w.P, last_limbs, last_scale);
}

// true when the pre-conditioner (pre, at) reading a latent of pitch ldx runs on the row-resident kernel AND can take the previous layer's folded
// ActNorm + permuter `lu` as its pre-layer (premlp.hip): decided once per layer pair by flow_forward, which then skips that layer's GEMM launch
static bool attention_takes_lu(const fc_flow& f, const PackedMLP& pre, const AttnPack& at, const PackedLinear& lu, const FlowWs& w, int act) {
    const Dims& d = f.d;
    return premlp_fusable(pre.in_layer, pre.mid, pre.out_layer, at.q) && d.ldx >= pre.in_layer.K_pad &&
           premlp_rows_ok(w.P_pad, d.I_pad, w.q, w.h[0], (size_t)w.P_pad * d.ldh()) && premlp_lu_fusable(lu, pre.in_layer, act, d.ldx);
}

// Attention probe (fc_flow_attention_weights_f32): the softmax rows of the selected target points at the requested attentions, written by
// attention_weights.hip next to the layer's attention launch.  Layer id -1 = the augmenter's attention, l >= 0 = flow layer l's pre-conditioner.
// Owns its tables: a pass deferred by the range check may run again after the entry point has returned.
struct AttnProbe {
    std::vector<int> layers;
    std::vector<float*> out;        // one [B][P][M] device buffer per entry of `layers`
    const int32_t* sel = nullptr;   // device [P] or [B][P]; null = all N points
    int P = 0, sel_per_scene = 0;
    // the second kind of request (fc_flow_attention_mass_f32, attention_mass.hip): the weighted column sums of the same rows over all N points
    std::vector<int> mass_layers;
    std::vector<float*> mass_out;            // one [B][M] device buffer per entry of `mass_layers`
    const float* row_weight = nullptr;       // device [B][N], or null = ones
    float* slab = nullptr;                   // attention_mass_slab_bytes(B, N, M) behind the forward's workspace plan; every layer reuses it (stream order)
};
constexpr int kNoProbeLayer = -2;

// Where this pass's keys and values are.  Built per pass, never kept: w.ctx16 and w.kv_limbs differ between the fast pass and its bf16-limb
// repeat (prepare), and a deferred pass may run after the entry point has returned.
static AttnKeys attention_keys(const fc_flow& f, const FlowWs& w, const AttnPack& at) {
    const Dims& d = f.d;
    if (w.ctx16) return AttnKeys::context(w.ctx16);                                         // K|V fold, split-fp16 scope: the context limb image
    if (f.kv_fold) return AttnKeys::panels(w.ctxp, d.E_pad, w.ctxp, d.E_pad, nullptr);      // K|V fold, fp32: the context panel itself
    if (w.kv_limbs) return AttnKeys::slice(reinterpret_cast<const unsigned short*>(w.kv), w.ldkv, at.kv_col);
    return AttnKeys::panels(w.kv + at.kv_col, w.ldkv, w.kv + at.kv_col + d.I_pad, w.ldkv, w.kv16);
}

// pre-conditioner: pre-MLP -> LayerNorm -> q -> attention; result in w.a  (models/cif_block.py:14-20 / augmenter.py:15-16)
static void run_attention(const fc_flow& f, const PackedMLP& pre, const AttnPack& at, const ASeg& in, FlowWs& w, int act, int B, int N, int M,
                          hipStream_t s, const PackedLinear* lu = nullptr, const float* xprev = nullptr, const AttnProbe* probe = nullptr,
                          int probe_layer = kNoProbeLayer) {
    const Dims& d = f.d;
    const int ldh = d.ldh();
    const AttnKeys keys = attention_keys(f, w, at);
    // q is complete in w.q (`lq` null) or up to rstd and the bias, which the limb-image kernels apply on load: probe if asked, then attend
    auto attend = [&](const AttnLnq* lq) {
        const AttnQuery qy{w.q, d.I_pad, 1.0f, lq};
        const AttnProblem pb{B, N, N, M, M, d.I_pad, w.m_counts};
        if (probe)
            for (size_t i = 0; i < probe->layers.size(); ++i)
                if (probe->layers[i] == probe_layer) launch_attention_weights(qy, keys, pb, probe->sel, probe->P, probe->sel_per_scene, probe->out[i], s);
        if (probe)
            for (size_t i = 0; i < probe->mass_layers.size(); ++i)
                if (probe->mass_layers[i] == probe_layer) launch_attention_mass(qy, keys, pb, probe->row_weight, probe->slab, probe->mass_out[i], s);
        launch_attention(qy, keys, pb, w.a, d.I_pad, s);
    };
    if (premlp_fusable(pre.in_layer, pre.mid, pre.out_layer, at.q) && in.lda >= pre.in_layer.K_pad &&
        premlp_rows_ok(w.P_pad, d.I_pad, w.q, w.h[0], (size_t)w.P_pad * ldh)) {
        // the whole chain x1 -> MLP -> LayerNorm -> q in one kernel: the activations stay in registers (premlp.hip); with `lu` the
        // previous layer's ActNorm + LU runs in front of it and writes this layer's latent (in.ptr) from xprev
        launch_premlp(in.ptr, in.lda, pre.in_layer, pre.mid, pre.out_layer, at.q, act, w.q, d.I_pad, w.P_pad, w.P, s, w.h[0], (size_t)w.P_pad * ldh, lu, xprev);
    } else {
        if (lu) throw Error(FC_ERR_INVALID, "run_attention: a pending ActNorm + LU pre-layer needs the row-resident pre-attention kernel");
        const int cur = run_mlp_hidden(f, pre, &in, nullptr, w, act, s);
        if (at.has_lnq && gemm_lnq_ok()) {
            // out_layer, LayerNorm and the q projection as ONE GEMM (AttnPack::lnq) + a 16 MB finalize pass
            GemmEpi e{};
            e.C = w.q; e.ldc = d.I_pad; e.d2 = d.A_in; e.ldj_part = w.lnss; e.ldj_pitch = (size_t)w.P_pad; e.rows_valid = w.P;
            ASeg a{w.h[cur], ldh};
            launch_gemm(at.lnq, &a, w.P_pad, e, EPI_LNQ, s);
            if (keys.form != AttnKeys::PANELS) {
                // the attention kernel applies rstd and the bias while it loads its queries
                const AttnLnq lq{w.lnss, d.A_in / 64, (size_t)w.P_pad, 1.0f / (float)d.A_in, at.q_bias};
                attend(&lq);
            } else {
                launch_lnq_finalize(w.q, d.I_pad, w.lnss, d.A_in / 64, (size_t)w.P_pad, d.A_in, at.q_bias, w.P, s);
                attend(nullptr);
            }
            return;
        }
        int o = 0;
        while (o == cur) ++o;
        ASeg a{w.h[cur], ldh};
        launch_gemm(pre.out_layer, &a, w.P_pad, linear_epi(w.h[o], ldh, w.P), EPI_LINEAR, s);
        launch_layernorm(w.h[o], ldh, d.A_in, w.P, s);
        ASeg aq{w.h[o], ldh};
        launch_gemm(at.q, &aq, w.P_pad, linear_epi(w.q, d.I_pad, w.P), EPI_LINEAR, s);
    }
    attend(nullptr);
}

// the conditioned coupling of one block (PreConditionApplier, models/transform.py:47-58), forward or inverse, in place on xc
static void run_coupling(fc_flow& f, const BlockPack& b, FlowWs& w, float* xc, const float* rowscal, float* logprob, bool inverse, int B, int N,
                         int M, hipStream_t s, const PackedLinear* lu = nullptr, const float* xprev = nullptr, int trace_layer = -1,
                         const AttnProbe* probe = nullptr) {
    const Dims& d = f.d;
    const fc_flow_config& c = f.cfg;
    ASeg segs[2];
    segs[0] = {xc, d.ldx};
    if (b.has_attn) {
        // CIFblock builds its pre_attention_mlp with GELU regardless of the configured nonlinearity (cif_block.py:61)
        run_attention(f, b.pre, b.attn, segs[0], w, b.has_cif ? (int)FC_ACT_GELU : c.nonlinearity, B, N, M, s, lu, xprev, probe,
                      trace_layer >= 0 ? trace_layer : kNoProbeLayer);
        segs[1] = {w.a, d.I_pad};
    } else {
        if (lu) throw Error(FC_ERR_INVALID, "run_coupling: a pending ActNorm + LU pre-layer needs an attention pre-conditioner");
        segs[1] = {w.ctxp, d.E_pad};
    }
    if (trace_layer >= 0 && t_flow_trace) {
        // diagnostic trace (fc_debug_flow_trace): the x2 half exactly as this coupling will read it (behind a fused ActNorm + LU pre-layer)
        if ((size_t)(trace_layer + 1) * w.P * d.d2 > t_flow_trace_floats) throw Error(FC_ERR_INVALID, "fc_debug_flow_trace: buffer too small for n_flow_layers x rows x d2");
        FC_HIP(hipMemcpy2DAsync(t_flow_trace + (size_t)trace_layer * w.P * d.d2, (size_t)d.d2 * 4, xc + d.d1_pad, (size_t)d.ldx * 4, (size_t)d.d2 * 4, (size_t)w.P,
                                hipMemcpyDeviceToDevice, s));
    }
    // limb chain: the spline parameter GEMM spans 30 column tiles that would each re-split the same fp32 rows into fp16 limbs; the
    // layer before it writes its output once as the limb image instead (GemmEpi::C16) and the parameter GEMM copies it (A16)
    const bool fused_spline = c.flow_type == FC_FLOW_SPLINE && !inverse && gemm_split_enabled() && b.net.out_layer.W3 != nullptr;
    const PackedLinear& last_hidden = b.net.mid.empty() ? b.net.in_layer : b.net.mid.back();
    const bool chain = fused_spline && gemm_limb_chain_ok() && limb_chain_pair(last_hidden, b.net.out_layer) && last_hidden.N_pad > 64;
    // the same chain into the affine coupling's (s, t) layer: forward direction, split-fp16 scope, pair-packed epilogue on the DMA tile
    const bool chain_aff = c.flow_type == FC_FLOW_AFFINE && !inverse && gemm_limb_chain_all_ok() && limb_chain_pair(last_hidden, b.net.out_layer) &&
                           last_hidden.N_pad % 128 == 0 && !b.net.mid.empty();
    // round 4: the chain's last activation in the one-accumulator form (common.h kOneAccActScale) for the 256 x 256 fused spline kernel (spline_wide.hip)
    const bool wide = chain && gemm_spline_wide_on() && spline_wide_eligible(b.net.out_layer, c.num_bins_spline) && w.P_pad % 256 == 0;
    const int cur = run_mlp_hidden(f, b.net, segs, rowscal, w, c.nonlinearity, s, (chain || chain_aff) ? w.h16 : nullptr, wide ? kOneAccActScale : 0.f);
    ASeg a{(chain || chain_aff) ? w.h[0] : w.h[cur], d.ldh()};
    if (c.flow_type == FC_FLOW_AFFINE) {
        GemmEpi e{};
        e.xbuf = xc; e.ldx = d.ldx; e.x2_col0 = d.d1_pad; e.d2 = d.d2; e.scale_fn = c.affine_scale_fn;
        e.logprob = logprob; e.rows_valid = w.P; e.inverse = inverse;
        if (!inverse) w.ldj_into(e);
        if (chain_aff) e.A16 = w.h16;
        launch_gemm(b.net.out_layer, &a, w.P_pad, e, EPI_AFFINE, s);
    } else if (fused_spline) {
        // forward: the parameter GEMM evaluates the splines in its epilogue; only per-tile log-det partials leave the kernel
        GemmEpi e{};
        e.xbuf = xc; e.ldx = d.ldx; e.x2_col0 = d.d1_pad; e.d2 = d.d2; e.spline_K = c.num_bins_spline; e.rows_valid = w.P;
        w.ldj_into(e);
        if (chain) { e.A16 = w.h16; e.a16_scale = wide ? kOneAccActScale : 0.f; }
        launch_gemm(b.net.out_layer, &a, w.P_pad, e, EPI_SPLINE, s);       // log-dets accumulate in w.ldjp; flow_forward reduces them once
    } else if (expm_wide(f)) {
        // parameter panel in row chunks: out-layer GEMM of the chunk into w.spl, then the matrix-exponential action of its points
        for (int r0 = 0; r0 < w.P; r0 += w.spl_rows) {
            const int rows_alloc = std::min(w.spl_rows, w.P_pad - r0);
            const int rows_valid = std::min(rows_alloc, w.P - r0);
            ASeg ac{a.ptr + (size_t)r0 * a.lda, a.lda};
            launch_gemm(b.net.out_layer, &ac, rows_alloc, linear_epi(w.spl, d.ldp, rows_valid), EPI_LINEAR, s);
            float* x2 = xc + (size_t)r0 * d.ldx + d.d1_pad;
            float* info = t_expm_info && trace_layer >= 0 && (size_t)(trace_layer + 1) * w.P * 4 <= t_expm_info_floats
                              ? t_expm_info + ((size_t)trace_layer * w.P + r0) * 4 : nullptr;
            launch_expm_wide(w.spl, d.ldp, x2, d.ldx, b.expm_scal, x2, d.ldx, d.d2, inverse ? nullptr : logprob + r0, inverse ? 0 : 2, rows_valid, d.d2,
                             inverse, f.expm_status, info, s);
        }
    } else {
        launch_gemm(b.net.out_layer, &a, w.P_pad, linear_epi(w.spl, d.ldp, w.P), EPI_LINEAR, s);
        if (c.flow_type == FC_FLOW_SPLINE)
            launch_spline(w.spl, d.ldp, xc, d.ldx, d.d1_pad, d.d2, c.num_bins_spline, logprob, w.P, inverse, s);
        else
            launch_expm_coupling(w.spl, d.ldp, xc, d.ldx, d.d1_pad, d.d2, b.expm_scal, logprob, w.P, inverse, s);
    }
}

// CIF: net(x) -> [mean | log_std] pairs with the given pair epilogue
static void run_cif_dist(fc_flow& f, const CifPack& cp, FlowWs& w, float* xc, GemmEpi e, int epi, hipStream_t s) {
    ASeg in{xc, f.d.ldx};
    const int cur = run_mlp_hidden(f, cp.dist, &in, nullptr, w, FC_ACT_GELU, s);
    ASeg a{w.h[cur], f.d.ldh()};
    e.clamp = f.cfg.clamp_dist; e.d2 = f.d.nz; e.rows_valid = w.P;
    if (!e.inverse) w.ldj_into(e);
    launch_gemm(cp.dist.out_layer, &a, w.P_pad, e, epi, s);
}
static void run_cif_affine(fc_flow& f, const CifPack& cp, FlowWs& w, float* xc, float* logprob, bool inverse, hipStream_t s) {
    const Dims& d = f.d;
    ASeg in{w.cbuf, d.nz_pad};
    const int cur = run_mlp_hidden(f, cp.aff, &in, nullptr, w, FC_ACT_GELU, s);
    ASeg a{w.h[cur], d.ldh()};
    GemmEpi e{};
    e.xbuf = xc; e.ldx = d.ldx; e.x2_col0 = 0; e.split = d.d1; e.split_pad = d.d1_pad; e.d2 = d.D; e.scale_fn = FC_SCALE_SIGMOID;
    e.post_scale = cp.post_scale; e.logprob = logprob; e.rows_valid = w.P; e.inverse = inverse;
    if (!inverse) w.ldj_into(e);
    launch_gemm(cp.aff.out_layer, &a, w.P_pad, e, EPI_AFFINE, s);
}

// a dense [rows, D] tensor into the x layout [x1 | 0-pad | x2 | 0-pad] (the pads are the caller's zero fill)
static void load_x_layout(const float* src, float* xc, const Dims& d, int rows, hipStream_t s) {
    launch_pack_rows(src, d.D, d.d1, xc, d.ldx, 0, d.d1, rows, s);
    launch_pack_rows(src + d.d1, d.D, d.d2, xc, d.ldx, d.d1_pad, d.d2, rows, s);
}
// a block's folded ActNorm + permuter (or its inverse) from the latent xc into the other buffer, which becomes the latent
static void apply_lin(const PackedLinear& lin, const Dims& d, const FlowWs& w, float*& xc, float*& xn, hipStream_t s) {
    ASeg ax{xc, d.ldx};
    launch_gemm(lin, &ax, w.P_pad, linear_epi(xn, d.ldx, w.P), EPI_LINEAR, s);
    std::swap(xc, xn);
}

struct Prep {
    FlowWs w;
    const float* rowscal = nullptr;
};
static Prep prepare(fc_flow& f, const float* ctx, const int32_t* ctx_counts, const float* extra, int B, int N, int M, void* ws, size_t ws_bytes, hipStream_t s) {
    const Dims& d = f.d;
    const fc_flow_config& c = f.cfg;
    if (B < 1 || N < 1 || M < 1) throw Error(FC_ERR_INVALID, "B, N, M must be positive");
    if (!ctx) throw Error(FC_ERR_INVALID, "null ctx");
    if (d.X && !extra) throw Error(FC_ERR_INVALID, "this flow was built with extra context: extra must not be NULL");
    if (c.global_context && M != N) throw Error(FC_ERR_INVALID, "global context is per target point: ctx must be [B,N,E] (M == N)");
    Prep p;
    p.w = plan_ws(f, B, N, M, ws, ws_bytes, false, nullptr);
    FlowWs& w = p.w;
    w.m_counts = ctx_counts;
    launch_pack_rows(ctx, d.E, d.E, w.ctxp, d.E_pad, 0, d.E_pad, w.Pc, s);
    // per-scene counts: a scene's rows beyond its count are padding the caller may have left anything in.  No attention reads them as keys,
    // but the limb image and the K|V projection below take every row: zeroed here for the reason given for the panel's tail
    launch_zero_pad_rows(w.ctxp, d.E_pad, ctx_counts, B, M, s);
    // pad rows of the context panel: the K|V projection stages them like any row, and stale workspace bytes there (a NaN, a value beyond fp16's
    // range) would raise the split-fp16 range flag -- a needless repeat of the whole pass on the bf16 limbs, and a scene whose log-probs then
    // depend on what ran in the workspace before (found in round 4: one scene of 200 context points behind a three-scene batch)
    if (w.Pc_pad > w.Pc) launch_fill(w.ctxp + (size_t)w.Pc * d.E_pad, 0.f, (size_t)(w.Pc_pad - w.Pc) * d.E_pad, s);
    // pad rows of the attention output: the attention kernels write the P valid rows only, and the coupling net's in_layer GEMM stages all P_pad
    // rows of w.a as an operand segment.  Stale workspace bytes there (the limb image of a call with another batch size, read as fp32) raised the
    // range flag and repeated every later pass on the bf16 limbs: seen with the stacked K|V projection (knob 33 = 0), a 4-scene call after
    // 1-scene calls on the same workspace (tests/test_gpu_context_counts.py compares exactly such calls)
    if (f.n_attn && w.P_pad > w.P) launch_fill(w.a + (size_t)w.P * d.I_pad, 0.f, (size_t)(w.P_pad - w.P) * d.I_pad, s);
    if (d.X) { launch_repeat_extra(extra, d.X, w.rowscal, B, N, s); p.rowscal = w.rowscal; }
    if (f.n_attn && f.kv_fold) {
        // keys = values = the context panel: one limb image per forward for the split-fp16 attention (range flag as the projection's epilogue
        // raised it); the fp32-input attention (attn_fp16, knob 5, = 0; the bf16-limb repeat of a pass) reads the panel itself
        if (gemm_fp16_flag() && g_knobs.attn_fp16 && d.I_pad <= 64) {
            launch_context_limbs(w.ctxp, d.E_pad, reinterpret_cast<unsigned short*>(w.kv16), w.Pc, d.I_pad, s);
            w.ctx16 = reinterpret_cast<const unsigned short*>(w.kv16);
        }
    } else if (f.n_attn) {
        // inside a guard scope the stacked K|V projection writes its output straight as the limb image the split-fp16 attention
        // stages (same bytes, same buffer): no fp32 K/V, no per-layer conversion pass
        w.kv_limbs = gemm_limb_chain_ok() && g_knobs.attn_fp16 && d.I_pad <= 64 && f.kv_all.W2 != nullptr && w.ldkv % 128 == 0 && w.ldkv == f.kv_all.N_pad;
        GemmEpi e{};
        e.rows_valid = w.Pc;
        if (w.kv_limbs) { e.C16 = reinterpret_cast<unsigned short*>(w.kv); e.c16_scale = kOneAccActScale; }      // (the one-accumulator image the attention kernel multiplies)
        else { e.C = w.kv; e.ldc = w.ldkv; }
        ASeg a{w.ctxp, d.E_pad};
        launch_gemm(f.kv_all, &a, w.Pc_pad, e, EPI_LINEAR, s);
    }
    if (d.nz > 0) launch_fill(w.cbuf, 0.f, (size_t)w.P_pad * d.nz_pad, s);
    return p;
}

static int expected_noise(const fc_flow& f) { return (f.has_augment ? 1 : 0) + (f.d.nz > 0 ? f.cfg.n_flow_layers : 0); }

static void flow_forward(fc_flow& f, const float* x, const float* ctx, const int32_t* ctx_counts, const float* extra, const float* const* eps, int n_eps,
                         float* logprob, float* z_out, int B, int N, int M, void* ws, size_t ws_bytes, hipStream_t s, const AttnProbe* probe = nullptr) {
    const Dims& d = f.d;
    const fc_flow_config& c = f.cfg;
    if (!x || (!logprob && !probe)) throw Error(FC_ERR_INVALID, "null x / logprob");
    if (n_eps != expected_noise(f)) throw Error(FC_ERR_INVALID, "wrong number of noise tensors");
    for (int i = 0; i < n_eps; ++i) if (!eps || !eps[i]) throw Error(FC_ERR_INVALID, "null noise tensor");
    Prep pr = prepare(f, ctx, ctx_counts, extra, B, N, M, ws, ws_bytes, s);
    FlowWs& w = pr.w;
    if (!logprob) logprob = w.lp_scratch;          // (a probe call that wants no log-prob: the pass still accumulates one)
    if (f.expm_status) FC_HIP(hipMemsetAsync(f.expm_status, 0, sizeof(int), s));
    int eps_i = 0;

    launch_fill(logprob, 0.f, (size_t)w.P, s);
    const int ldj_tiles = w.ldj_slots;                                         // epilogues accumulate their log-det partials here
    if (ldj_tiles) launch_fill(w.ldjp, 0.f, (size_t)ldj_tiles * w.P_pad, s);
    float* xc = w.xa;
    float* xn = w.xb;
    launch_fill(xc, 0.f, (size_t)w.P_pad * d.ldx, s);
    if (f.has_augment) {
        launch_pack_rows(x, d.Din, d.Din, w.xin, 32, 0, 32, w.P, s);
        if (w.P_pad > w.P) launch_fill(w.xin + (size_t)w.P * 32, 0.f, (size_t)(w.P_pad - w.P) * 32, s);      // (pad rows: zeros, not stale workspace bytes)
        const int n1 = std::min(d.Din, d.d1);                                       // latent[0:Din] = x, split over the x1 | x2 regions
        launch_pack_rows(x, d.Din, n1, xc, d.ldx, 0, n1, w.P, s);
        if (d.Din > n1) launch_pack_rows(x + n1, d.Din, d.Din - n1, xc, d.ldx, d.d1_pad, d.Din - n1, w.P, s);
        ASeg in{w.xin, 32};
        run_attention(f, f.aug_pre, f.aug_attn, in, w, c.nonlinearity, B, N, M, s, nullptr, nullptr, probe, -1);
        ASeg segs[2] = {{w.xin, 32}, {w.a, d.I_pad}};
        const int cur = run_mlp_hidden(f, f.aug_net, segs, pr.rowscal, w, c.nonlinearity, s);
        GemmEpi e{};
        e.xbuf = xc; e.ldx = d.ldx; e.d2 = d.D - d.Din; e.logprob = logprob; e.eps = eps[eps_i++];
        e.d_in = d.Din; e.d1 = d.d1; e.d1_pad = d.d1_pad; e.rows_valid = w.P;
        w.ldj_into(e);
        ASeg a{w.h[cur], d.ldh()};
        launch_gemm(f.aug_net.out_layer, &a, w.P_pad, e, EPI_AUGMENT, s);
    } else {
        load_x_layout(x, xc, d, w.P, s);
    }
    const PackedLinear* pend = nullptr;
    for (int l = 0; l < c.n_flow_layers; ++l) {
        BlockPack& b = f.blocks[l];
        if (b.has_cif) {
            GemmEpi ea{};                                   // Augment: z2 -> cbuf (natural order), ldj -= log N(z2)
            ea.xbuf = w.cbuf; ea.ldx = d.nz_pad; ea.d_in = 0; ea.d1 = d.nz; ea.d1_pad = d.nz_pad; ea.logprob = logprob; ea.eps = eps[eps_i++];
            run_cif_dist(f, b.cif, w, xc, ea, EPI_AUGMENT, s);
            run_cif_affine(f, b.cif, w, xc, logprob, false, s);
            GemmEpi es{};                                   // Slice: ldj += log N(actnorm(z2); mu(zx), sigma(zx))
            es.val = w.cbuf; es.ldval = d.nz_pad; es.val_shift = b.cif.z2_shift; es.val_scale = b.cif.z2_scale; es.logprob = logprob;
            run_cif_dist(f, b.cif, w, xc, es, EPI_SLICE, s);
        }
        // `pend`: the previous layer's folded ActNorm + permuter, not launched yet -- it runs as the pre-layer of this layer's row-resident
        // pre-attention kernel, reading xc and writing xn, which becomes this layer's latent
        if (pend) std::swap(xc, xn);
        run_coupling(f, b, w, xc, pr.rowscal, logprob, false, B, N, M, s, pend, pend ? xn : nullptr, l, probe);
        pend = nullptr;
        if (b.has_lin) {
            const bool next_takes_it = l + 1 < c.n_flow_layers && f.blocks[l + 1].has_attn && !f.blocks[l + 1].has_cif &&
                                       attention_takes_lu(f, f.blocks[l + 1].pre, f.blocks[l + 1].attn, b.lin, w, c.nonlinearity);
            if (next_takes_it) pend = &b.lin;
            else apply_lin(b.lin, d, w, xc, xn, s);
        }
    }
    if (pend) throw Error(FC_ERR_INVALID, "flow_forward: an ActNorm + LU pre-layer was left pending");
    if (ldj_tiles) launch_ldj_reduce(w.ldjp, ldj_tiles, (size_t)w.P_pad, logprob, w.P, s);
    launch_base_density(xc, d.ldx, d.d1, d.d1_pad, d.d2, logprob, (float)f.log_const, z_out, d.D, w.P, s);
}

// Flow.sample's inverse pass (models/transform.py:79-84): transforms in reverse order, each inverted.
static void flow_inverse(fc_flow& f, const float* z, const float* ctx, const float* extra, const float* const* eps, int n_eps, float* x_out,
                         int B, int N, int M, void* ws, size_t ws_bytes, hipStream_t s) {
    const Dims& d = f.d;
    const fc_flow_config& c = f.cfg;
    if (!z || !x_out) throw Error(FC_ERR_INVALID, "null z / x_out");
    const int need_eps = d.nz > 0 ? c.n_flow_layers : 0;     // Slice.inverse draws once per CIF block (models/slice.py:46-58)
    if (n_eps != need_eps) throw Error(FC_ERR_INVALID, "wrong number of noise tensors for the inverse pass");
    for (int i = 0; i < n_eps; ++i) if (!eps || !eps[i]) throw Error(FC_ERR_INVALID, "null noise tensor");
    ensure_lin_inverse(f);
    Prep pr = prepare(f, ctx, nullptr, extra, B, N, M, ws, ws_bytes, s);      // (one scene is never ragged, and make_sample passes one)
    FlowWs& w = pr.w;
    if (f.expm_status) FC_HIP(hipMemsetAsync(f.expm_status, 0, sizeof(int), s));
    float* xc = w.xa;
    float* xn = w.xb;
    launch_fill(xc, 0.f, (size_t)w.P_pad * d.ldx, s);
    load_x_layout(z, xc, d, w.P, s);
    int eps_i = 0;
    for (int l = c.n_flow_layers - 1; l >= 0; --l) {
        BlockPack& b = f.blocks[l];
        if (b.has_lin) apply_lin(b.lin_inv, d, w, xc, xn, s);
        run_coupling(f, b, w, xc, pr.rowscal, nullptr, true, B, N, M, s);
        if (b.has_cif) {
            GemmEpi ea{};                                   // Slice.inverse: x2n ~ N(mu(z), sigma(z)); stored as z2 = x2n / g2 + shift2
            ea.xbuf = w.cbuf; ea.ldx = d.nz_pad; ea.d_in = 0; ea.d1 = d.nz; ea.d1_pad = d.nz_pad; ea.eps = eps[eps_i++]; ea.inverse = 1;
            ea.val_shift = b.cif.z2_shift; ea.val_scale = b.cif.z2_scale;
            run_cif_dist(f, b.cif, w, xc, ea, EPI_AUGMENT, s);
            run_cif_affine(f, b.cif, w, xc, nullptr, true, s);
        }
    }
    // Augment.inverse keeps the first input_dim latent dims (models/augmenter.py:65-67)
    const int n1 = std::min(d.Din, d.d1);
    launch_pack_rows(xc, d.ldx, n1, x_out, d.Din, 0, n1, w.P, s);
    if (d.Din > n1) launch_pack_rows(xc + d.d1_pad, d.ldx, d.Din - n1, x_out, d.Din, n1, d.Din - n1, w.P, s);
}

// the wide ExponentialCoupling kernel's status word, read back after a pass (a synchronisation, paid by those flows only): a point whose
// matrix exceeds the kernel's bound fails the call instead of returning a truncated series
static void check_expm_status(const fc_flow& f, hipStream_t s) {
    if (!f.expm_status) return;
    int h = 0;
    FC_HIP(hipMemcpyAsync(&h, f.expm_status, sizeof(int), hipMemcpyDeviceToHost, s));
    FC_HIP(hipStreamSynchronize(s));
    if (h) throw Error(FC_ERR_UNSUPPORTED, "ExponentialCoupling: a coupling matrix norm ||W - mu I||_1 exceeds the matrix-exponential kernel's bound "
                                           "(40 Taylor steps, 534): the result would be a truncated series");
}

}  // namespace fc

extern "C" {

int fc_flow_create(const fc_flow_config* cfg, const fc_tensor* tensors, int32_t n_tensors, fc_flow** out) {
    FC_API_BEGIN
    if (!cfg || !out) throw fc::Error(FC_ERR_INVALID, "fc_flow_create: null argument");
    *out = nullptr;
    std::unique_ptr<fc_flow> f(new fc_flow());
    f->cfg = *cfg;
    fc::WeightTable wt(tensors, n_tensors);
    fc::build_flow(*f, wt);
    f->fp16_flag = (int*)f->arena.alloc_floats(1);
    if (fc::expm_wide(*f)) f->expm_status = (int*)f->arena.alloc_floats(1);
    FC_HIP(hipDeviceSynchronize());
    *out = f.release();
    FC_API_END
}

void fc_flow_destroy(fc_flow* flow) { delete flow; }

int fc_flow_workspace_bytes(const fc_flow* flow, int32_t B, int32_t N, int32_t M, size_t* bytes) {
    FC_API_BEGIN
    if (!flow || !bytes || B < 1 || N < 1 || M < 1) throw fc::Error(FC_ERR_INVALID, "fc_flow_workspace_bytes: bad argument");
    fc::plan_ws(*flow, B, N, M, nullptr, 0, true, bytes);
    FC_API_END
}

int fc_flow_noise_count(const fc_flow* flow) { return flow ? fc::expected_noise(*flow) : 0; }
int fc_flow_noise_width(const fc_flow* flow, int32_t i) {
    if (!flow || i < 0 || i >= fc::expected_noise(*flow)) return 0;
    if (flow->has_augment && i == 0) return flow->d.D - flow->d.Din;
    return flow->d.nz;
}

// One guarded forward pass: fast split-fp16 GEMMs first; the whole pass is repeated with the bf16-limb GEMMs if an activation left fp16's
// range, which rewrites every output of the pass (log-probs, latent, weight buffers, slabs, masses).  With a deferred range check
// (fc_range_check_defer) the pass may be repeated after the entry point has returned, so it owns its arguments: the noise pointers and the
// probe are copied.  probe: null = a plain log-prob pass.  ctx_counts: null, or the per-scene context point counts of the *_counts_* entries.
static void guarded_forward(fc_flow* flow, const float* x, const float* ctx, const int32_t* ctx_counts, const float* extra, const float* const* eps, int n_eps,
                            float* logprob, float* z_out, int B, int N, int M, void* ws, size_t ws_bytes, hipStream_t s, const fc::AttnProbe* probe = nullptr) {
    const std::vector<const float*> eps_own(eps, eps + (eps && n_eps > 0 ? n_eps : 0));
    const bool probing = probe != nullptr;
    const fc::AttnProbe probe_own = probing ? *probe : fc::AttnProbe();
    fc::run_fp16_guarded(flow->fp16_flag, s, [=] {
        fc::flow_forward(*flow, x, ctx, ctx_counts, extra, eps_own.data(), n_eps, logprob, z_out, B, N, M, ws, ws_bytes, s, probing ? &probe_own : nullptr);
    }, true);
    fc::check_expm_status(*flow, s);
}

// The entries of fcflow.h / fcflow_attention_mass.h and their namesakes of fcflow_context_counts.h are one body each: `who` is the entry's name
// (it opens every message), `counted` says which of the two it is.  The namesakes refuse what has no per-scene count.
static void check_entry(const char* who, const fc_flow* flow, const void* workspace, bool counted, const int32_t* ctx_counts) {
    if (!flow || !workspace) throw fc::Error(FC_ERR_INVALID, std::string(who) + ": null flow / workspace");
    if (!counted) return;
    if (!ctx_counts) throw fc::Error(FC_ERR_INVALID, std::string(who) + ": null ctx_counts (the entry without per-scene counts takes one M for the batch)");
    if (flow->cfg.global_context)
        throw fc::Error(FC_ERR_INVALID, std::string(who) + ": this flow has a global context (ctx is per target point, [B,N,E]): there are no per-scene context point counts");
}

static void logprob_entry(const char* who, bool counted, fc_flow* flow, const float* x, const float* ctx, const int32_t* ctx_counts, const float* extra,
                          const float* const* eps, int32_t n_eps, float* logprob, float* z_out, int32_t B, int32_t N, int32_t M, void* workspace,
                          size_t workspace_bytes, void* stream) {
    check_entry(who, flow, workspace, counted, ctx_counts);
    guarded_forward(flow, x, ctx, ctx_counts, extra, eps, n_eps, logprob, z_out, B, N, M, workspace, workspace_bytes, (hipStream_t)stream);
}

int fc_flow_logprob_f32(fc_flow* flow, const float* x, const float* ctx, const float* extra, const float* const* eps, int32_t n_eps,
                        float* logprob, float* z_out, int32_t B, int32_t N, int32_t M, void* workspace, size_t workspace_bytes, void* stream) {
    FC_API_BEGIN
    logprob_entry("fc_flow_logprob_f32", false, flow, x, ctx, nullptr, extra, eps, n_eps, logprob, z_out, B, N, M, workspace, workspace_bytes, stream);
    FC_API_END
}

int fc_flow_logprob_counts_f32(fc_flow* flow, const float* x, const float* ctx, const int32_t* ctx_counts, const float* extra, const float* const* eps,
                               int32_t n_eps, float* logprob, float* z_out, int32_t B, int32_t N, int32_t M, void* workspace, size_t workspace_bytes,
                               void* stream) {
    FC_API_BEGIN
    logprob_entry("fc_flow_logprob_counts_f32", true, flow, x, ctx, ctx_counts, extra, eps, n_eps, logprob, z_out, B, N, M, workspace, workspace_bytes, stream);
    FC_API_END
}

// every request of a probe call is checked before anything is launched: layer ids -1 (augmenter) and 0 .. n_flow_layers - 1 with an attention
static void check_probe_layer(const fc_flow* flow, const std::string& who, int l) {
    if (l == -1) {
        if (!flow->has_augment)
            throw fc::Error(FC_ERR_INVALID, who + ": layer -1 (the augmenter's attention) does not exist: this flow's first transform "
                                            "is IdentityTransform (latent_dim == input_dim)");
    } else if (l < 0 || l >= flow->cfg.n_flow_layers) {
        throw fc::Error(FC_ERR_INVALID, who + ": layer id " + std::to_string(l) + " is out of range: valid ids are -1 (augmenter) and 0 .. " +
                                        std::to_string(flow->cfg.n_flow_layers - 1));
    } else if (!flow->blocks[l].has_attn) {
        throw fc::Error(FC_ERR_INVALID, who + ": flow layer " + std::to_string(l) + " has no attention: a global-context flow hands the "
                                        "embedding to its couplings directly (only layer -1, the augmenter, attends)");
    }
}
// the request list of probe entry `who` into a probe's (layers, output buffers) pair
static void probe_requests(const fc_flow* flow, const std::string& who, const int32_t* layers, float* const* out, int n_layers,
                           std::vector<int>& probe_layers, std::vector<float*>& probe_out) {
    for (int i = 0; i < n_layers; ++i) {
        if (!out[i]) throw fc::Error(FC_ERR_INVALID, who + ": null output buffer for request " + std::to_string(i));
        check_probe_layer(flow, who, layers[i]);
        probe_layers.push_back(layers[i]);
        probe_out.push_back(out[i]);
    }
}

static void attention_weights_entry(const char* who_c, bool counted, fc_flow* flow, const float* x, const float* ctx, const int32_t* ctx_counts,
                                    const float* extra, const float* const* eps, int32_t n_eps, const int32_t* layers, int32_t n_layers, const int32_t* sel,
                                    int32_t P, int32_t sel_per_scene, float* const* out, float* logprob, int32_t B, int32_t N, int32_t M, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const std::string who = who_c;
    check_entry(who_c, flow, workspace, counted, ctx_counts);
    if (n_layers < 1 || !layers || !out) throw fc::Error(FC_ERR_INVALID, who + ": no layers requested (layers / out are null or n_layers < 1)");
    if (!sel) P = N;
    if (P < 1) throw fc::Error(FC_ERR_INVALID, who + ": P must be positive");
    fc::AttnProbe probe;
    probe.sel = sel; probe.P = P; probe.sel_per_scene = sel ? (sel_per_scene != 0) : 0;
    probe_requests(flow, who, layers, out, n_layers, probe.layers, probe.out);
    guarded_forward(flow, x, ctx, ctx_counts, extra, eps, n_eps, logprob, nullptr, B, N, M, workspace, workspace_bytes, (hipStream_t)stream, &probe);
}

int fc_flow_attention_weights_f32(fc_flow* flow, const float* x, const float* ctx, const float* extra, const float* const* eps, int32_t n_eps,
                                  const int32_t* layers, int32_t n_layers, const int32_t* sel, int32_t P, int32_t sel_per_scene, float* const* out,
                                  float* logprob, int32_t B, int32_t N, int32_t M, void* workspace, size_t workspace_bytes, void* stream) {
    FC_API_BEGIN
    attention_weights_entry("fc_flow_attention_weights_f32", false, flow, x, ctx, nullptr, extra, eps, n_eps, layers, n_layers, sel, P, sel_per_scene, out, logprob,
                            B, N, M, workspace, workspace_bytes, stream);
    FC_API_END
}

int fc_flow_attention_weights_counts_f32(fc_flow* flow, const float* x, const float* ctx, const int32_t* ctx_counts, const float* extra,
                                         const float* const* eps, int32_t n_eps, const int32_t* layers, int32_t n_layers, const int32_t* sel, int32_t P,
                                         int32_t sel_per_scene, float* const* out, float* logprob, int32_t B, int32_t N, int32_t M, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    FC_API_BEGIN
    attention_weights_entry("fc_flow_attention_weights_counts_f32", true, flow, x, ctx, ctx_counts, extra, eps, n_eps, layers, n_layers, sel, P, sel_per_scene, out,
                            logprob, B, N, M, workspace, workspace_bytes, stream);
    FC_API_END
}

// the slab region of an attention-mass call sits behind the forward's workspace plan, which therefore stays what fc_flow_workspace_bytes reports
static size_t mass_slab_offset(const fc_flow& flow, int B, int N, int M) {
    size_t fwd = 0;
    fc::plan_ws(flow, B, N, M, nullptr, 0, true, &fwd);
    return (fwd + 255) / 256 * 256;
}

int fc_flow_attention_mass_workspace_bytes(const fc_flow* flow, int32_t B, int32_t N, int32_t M, size_t* bytes) {
    FC_API_BEGIN
    if (!flow || !bytes || B < 1 || N < 1 || M < 1) throw fc::Error(FC_ERR_INVALID, "fc_flow_attention_mass_workspace_bytes: bad argument");
    *bytes = mass_slab_offset(*flow, B, N, M) + fc::attention_mass_slab_bytes(B, N, M);
    FC_API_END
}

static void attention_mass_entry(const char* who_c, bool counted, fc_flow* flow, const float* x, const float* ctx, const int32_t* ctx_counts, const float* extra,
                                 const float* const* eps, int32_t n_eps, const int32_t* layers, int32_t n_layers, const float* row_weight, float* const* out,
                                 float* logprob, int32_t B, int32_t N, int32_t M, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string who = who_c;
    check_entry(who_c, flow, workspace, counted, ctx_counts);
    if (n_layers < 1 || !layers || !out) throw fc::Error(FC_ERR_INVALID, who + ": no layers requested (layers / out are null or n_layers < 1)");
    if (B < 1 || N < 1 || M < 1) throw fc::Error(FC_ERR_INVALID, "B, N, M must be positive");
    fc::AttnProbe probe;
    probe.row_weight = row_weight;
    probe_requests(flow, who, layers, out, n_layers, probe.mass_layers, probe.mass_out);
    const size_t slab_off = mass_slab_offset(*flow, B, N, M), need = slab_off + fc::attention_mass_slab_bytes(B, N, M);
    if (workspace_bytes < need)
        throw fc::Error(FC_ERR_WORKSPACE, who + ": workspace too small: " + std::to_string(workspace_bytes) + " bytes given, " + std::to_string(need) +
                                          " needed (fc_flow_attention_mass_workspace_bytes: the forward's workspace plus the slab region)");
    probe.slab = reinterpret_cast<float*>(static_cast<char*>(workspace) + slab_off);
    guarded_forward(flow, x, ctx, ctx_counts, extra, eps, n_eps, logprob, nullptr, B, N, M, workspace, slab_off, (hipStream_t)stream, &probe);
}

int fc_flow_attention_mass_f32(fc_flow* flow, const float* x, const float* ctx, const float* extra, const float* const* eps, int32_t n_eps,
                               const int32_t* layers, int32_t n_layers, const float* row_weight, float* const* out, float* logprob, int32_t B, int32_t N,
                               int32_t M, void* workspace, size_t workspace_bytes, void* stream) {
    FC_API_BEGIN
    attention_mass_entry("fc_flow_attention_mass_f32", false, flow, x, ctx, nullptr, extra, eps, n_eps, layers, n_layers, row_weight, out, logprob, B, N, M,
                         workspace, workspace_bytes, stream);
    FC_API_END
}

int fc_flow_attention_mass_counts_f32(fc_flow* flow, const float* x, const float* ctx, const int32_t* ctx_counts, const float* extra, const float* const* eps,
                                      int32_t n_eps, const int32_t* layers, int32_t n_layers, const float* row_weight, float* const* out, float* logprob,
                                      int32_t B, int32_t N, int32_t M, void* workspace, size_t workspace_bytes, void* stream) {
    FC_API_BEGIN
    attention_mass_entry("fc_flow_attention_mass_counts_f32", true, flow, x, ctx, ctx_counts, extra, eps, n_eps, layers, n_layers, row_weight, out, logprob, B, N, M,
                         workspace, workspace_bytes, stream);
    FC_API_END
}

int fc_flow_inverse_f32(fc_flow* flow, const float* z, const float* ctx, const float* extra, const float* const* eps, int32_t n_eps, float* x_out,
                        int32_t B, int32_t N, int32_t M, void* workspace, size_t workspace_bytes, void* stream) {
    FC_API_BEGIN
    if (!flow || !workspace) throw fc::Error(FC_ERR_INVALID, "fc_flow_inverse_f32: null flow / workspace");
    fc::flow_inverse(*flow, z, ctx, extra, eps, n_eps, x_out, B, N, M, workspace, workspace_bytes, (hipStream_t)stream);
    fc::check_expm_status(*flow, (hipStream_t)stream);
    FC_API_END
}

}  // extern "C"
