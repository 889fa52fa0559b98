// The entry points of the C ABI that are not about one engine: version, last error, the in-library profiler, the knobs and diagnostics, and the
// single-operator calls (fc_op_*): the SAME kernels the engines launch, wrapped so that unit-level parity tests can drive them with dense
// tensors.  These wrappers allocate temporary device memory for the padded layouts (they are test/diagnostic conveniences, not the hot path).
#include <cstring>
#include <memory>

#include "flow_model.h"
#include "spline.h"

namespace fc {

struct TmpBuf {
    void* p = nullptr;
    explicit TmpBuf(size_t bytes) { FC_HIP(hipMalloc(&p, bytes ? bytes : 4)); }
    ~TmpBuf() { (void)hipFree(p); }
    float* f() const { return (float*)p; }
};

Knobs g_knobs;

struct KnobEntry { int key; const char* name; int Knobs::*field; bool (*accepts)(int v); };
#define FC_KNOB_ENTRY(key, field, def, accept, doc) {key, #field, &Knobs::field, [](int v) { return accept; }},
static const KnobEntry kKnobTable[] = {FC_KNOBS(FC_KNOB_ENTRY)};
#undef FC_KNOB_ENTRY
static const KnobEntry* find_knob(int key) {
    for (const KnobEntry& k : kKnobTable) if (k.key == key) return &k;
    return nullptr;
}

// fc_debug_premlp_q_f32, path 0: which of the row-resident pre-attention kernel's conditions (premlp.hip) does not hold, by the predicate's name
// and, where the shapes tell, the reason.  The decision itself is the predicates'; this only words it.
static std::string premlp_refusal(const PackedMLP& m, const AttnPack& at, const Dims& d, bool fusable, bool rows_ok, bool pre, bool lu_ok,
                                  const PackedLinear& lu, int act, int D) {
    std::string r;
    auto add = [&](const std::string& t) { r += (r.empty() ? "" : "; ") + t; };
    if (!fusable) {
        std::string w = "premlp_fusable does not hold";
        if (!gemm_fp16_flag()) w += " (no split-fp16 guard scope: gemm_variant, knob 0, is not 5)";
        if (!g_knobs.premlp_fused) w += " (premlp_fused, knob 8, is 0)";
        if (m.mid.size() != 2) w += " (" + std::to_string(m.mid.size()) + " hidden layers, the kernel has two)";
        for (int h : m.sizes)
            if (h != 256) { w += " (hidden width " + std::to_string(h) + ", the kernel's is 256)"; break; }
        if (m.in_layer.K_pad > 256) w += " (the in_layer's input width k_in pads to " + std::to_string(m.in_layer.K_pad) + " columns, the kernel takes at most 256)";
        if (d.A_in != 256) w += " (attention input width " + std::to_string(d.A_in) + ", the kernel's is 256)";
        if (at.q.N_pad != 64) w += " (inner width I = " + std::to_string(d.I) + " pads to " + std::to_string(at.q.N_pad) + " q columns, the kernel writes 64)";
        bool images = m.in_layer.W2 && m.out_layer.W2 && at.q.W2;
        for (const PackedLinear& L : m.mid) images = images && L.W2;
        if (!images) w += " (a layer has no fp16 limb image: a weight beyond fp16's range)";
        add(w);
    }
    if (!rows_ok) add("premlp_rows_ok does not hold");
    if (pre && !lu_ok) {
        std::string w = "premlp_lu_fusable does not hold";
        if (!g_knobs.premlp_lu) w += " (premlp_lu, knob 26, is 0)";
        if (act != FC_ACT_GELU) w += " (activation code " + std::to_string(act) + ": the pre-layer kernel is instantiated for GELU only)";
        if (lu.K_pad != 320 || m.in_layer.K_pad != 160)
            w += " (latent width D = " + std::to_string(D) + " pads to " + std::to_string(lu.K_pad) + " columns, x1 to " + std::to_string(m.in_layer.K_pad) +
                 ": the pre-layer kernel takes 320 and 160)";
        if (!lu.W2) w += " (lu has no fp16 limb image: a weight beyond fp16's range)";
        add(w);
    }
    return r.empty() ? "the in_layer reads more columns than the staged panel has" : r;
}
}  // namespace fc

extern "C" {

int fc_abi_version(void) { return FC_ABI_VERSION; }
const char* fc_last_error(void) { return fc::get_last_error(); }

int fc_profile_enable(int32_t on) { fc::prof_set(on != 0); return FC_OK; }
int fc_profile_reset(void) { fc::prof_reset(); return FC_OK; }
int fc_profile_filter(const char* kernel_substr) { fc::prof_filter(kernel_substr); return FC_OK; }
int fc_profile_stride(int32_t n) { fc::prof_stride(n); return FC_OK; }
int fc_profile_report(char* buf, size_t cap) {
    FC_API_BEGIN
    const std::string r = fc::prof_report_json();
    if (!buf || cap < r.size() + 1) throw fc::Error(FC_ERR_INVALID, "fc_profile_report: buffer too small");
    memcpy(buf, r.c_str(), r.size() + 1);
    FC_API_END
}

/* the kernel-choice knobs of csrc/knobs.h by key (profiles/kernel_bench.py, bench.py --knob, the parity tests; not part of the stable ABI surface
   in fcflow.h on purpose).  An unknown or retired key is FC_ERR_INVALID; a value outside the knob's accepted set (a kernel variant that lost an
   A/B and was removed: DESIGN.md section 6) is refused with FC_ERR_UNSUPPORTED and leaves the setting as it was. */
int fc_debug_set(int32_t key, int32_t value) {
    const fc::KnobEntry* k = fc::find_knob(key);
    if (!k) return FC_ERR_INVALID;
    if (!k->accepts(value)) return FC_ERR_UNSUPPORTED;
    fc::g_knobs.*(k->field) = value;
    return FC_OK;
}
int fc_debug_get(int32_t key, int32_t* value) {
    const fc::KnobEntry* k = fc::find_knob(key);
    if (!k || !value) return FC_ERR_INVALID;
    *value = fc::g_knobs.*(k->field);
    return FC_OK;
}
int fc_debug_reset(void) { fc::g_knobs = fc::Knobs{}; return FC_OK; }      /* every knob back to its shipped default */
/* the knob's field name in csrc/knobs.h, or NULL for an unknown key (a script lists the table by walking the keys) */
const char* fc_debug_name(int32_t key) { const fc::KnobEntry* k = fc::find_knob(key); return k ? k->name : nullptr; }

/* diagnostic / test entry (not part of fcflow.h): out[rows, N] = x[rows, K] W[N, K]^T + bias through the ONE-ACCUMULATOR limb form on the 256 x 256 main loop of
   spline_wide.hip, nothing else -- the product the fused spline layer is built on, measurable against fp64 by itself; device pointers, wmax = max |W| */
int fc_debug_one_acc_gemm_f32(const float* x, const float* W, const float* bias, float wmax, float* out, int32_t rows, int32_t N, int32_t K, void* stream) {
    FC_API_BEGIN
    fc::one_acc_gemm_debug(x, W, bias, wmax, out, rows, N, K, (hipStream_t)stream);
    FC_API_END
}

/* host-side view of the spline parameter layer's column layout (csrc/spline.h) for the CPU tests: column of (transformed dim j, parameter
   pp) and the dim-major position inside a tile that the LDS-tile epilogues store a column at; no device call */
int32_t fc_debug_spline_col(int32_t j, int32_t pp, int32_t K) { return fc::spline_col(j, pp, K); }
int32_t fc_debug_spline_tile_pos(int32_t c, int32_t K) { return fc::spline_tile_pos(c, K); }

/* host-side view of the K|V fold's gate (flow_pack.cpp kv_fold_gate_dims) for the CPU tests: 1 when a flow whose attentions have this
   embedding width, inner width and these biases gets to_kv folded away at fc_flow_create (with kv_fold, knob 33, at its default); no device call */
int32_t fc_debug_kv_fold_gate(int32_t E, int32_t inner, int32_t q_bias, int32_t kv_bias) { return fc::kv_fold_gate_dims(E, inner, q_bias != 0, kv_bias != 0) ? 1 : 0; }

/* diagnostic (stamps, knob 20): copies the phase stamps of the last stamped fused-spline launch (16 x u64 per workgroup) to host memory; returns the count */
int64_t fc_debug_gemm_stamps(uint64_t* host, int64_t max_n) {
    try { return (int64_t)fc::gemm_read_stamps(reinterpret_cast<unsigned long long*>(host), (size_t)max_n); } catch (...) { return -1; }
}

/* deferred range check (include/fcflow.h) */
int fc_range_check_defer(int32_t on) {
    FC_API_BEGIN
    if (!on && fc::guard_pending()) fc::guard_resolve();
    fc::guard_set_deferred(on != 0);
    FC_API_END
}
int fc_range_check_resolve(int32_t* n_repeated) {
    FC_API_BEGIN
    const int n = fc::guard_resolve();
    if (n_repeated) *n_repeated = n;
    FC_API_END
}
int32_t fc_range_check_pending(void) { return fc::guard_pending(); }

/* diagnostic: trace of every coupling's x2 input of the calling thread's next fc_flow_logprob_f32 calls into a DEVICE buffer
   [n_flow_layers][B * N][d2] (flow_engine.cpp flow_set_trace); NULL switches it off.  Test infrastructure, not part of fcflow.h. */
int fc_debug_flow_trace(float* device_buf, int64_t capacity_floats) {
    fc::flow_set_trace(device_buf, device_buf && capacity_floats > 0 ? (size_t)capacity_floats : 0);
    return FC_OK;
}

/* diagnostic: while set, the wide ExponentialCoupling kernel of a forward pass writes {||W - mu I||_1, s, m, products} of every point of
 * layer l to device_buf[(l * rows + row) * 4 ...] (profiles: the norms and product counts a run saw) */
int fc_debug_expm_info(float* device_buf, int64_t capacity_floats) {
    fc::flow_set_expm_info(device_buf, device_buf && capacity_floats > 0 ? (size_t)capacity_floats : 0);
    return FC_OK;
}

/* number of calls that were repeated with the bf16-limb GEMMs because an activation left fp16's range (tests, diagnostics) */
int64_t fc_debug_fp16_fallbacks(void) { return (int64_t)fc::gemm_fp16_fallbacks(); }

int fc_op_linear_f32(const float* x, const float* W, const float* bias, const float* residual, float* y, int32_t rows, int32_t N, int32_t K,
                     int32_t act, void* stream) {
    FC_API_BEGIN
    using namespace fc;
    if (!x || !W || !y || rows < 1 || N < 1 || K < 1) throw Error(FC_ERR_INVALID, "fc_op_linear_f32: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int rp = round_up(rows, ROW_PAD), np = round_up(N, 32), kp = round_up(K, 32);
    const int na = gemm_n_alloc(np);
    TmpBuf xp((size_t)rp * kp * 4), wp((size_t)na * kp * 4), bp((size_t)na * 4), cp((size_t)rp * np * 4), rpad(residual ? (size_t)rp * np * 4 : 4);
    launch_fill(xp.f(), 0.f, (size_t)rp * kp, s);
    launch_fill(wp.f(), 0.f, (size_t)na * kp, s);
    launch_fill(bp.f(), 0.f, (size_t)na, s);
    launch_pack_rows(x, K, K, xp.f(), kp, 0, K, rows, s);
    launch_pack_rows(W, K, K, wp.f(), kp, 0, K, N, s);
    if (bias) launch_pack_rows(bias, N, N, bp.f(), np, 0, N, 1, s);
    if (residual) {
        launch_fill(rpad.f(), 0.f, (size_t)rp * np, s);
        launch_pack_rows(residual, N, N, rpad.f(), np, 0, N, rows, s);
    }
    PackedLinear L;
    L.W = wp.f(); L.bias = bp.f(); L.N_pad = np; L.K_pad = kp; L.nseg = 1; L.seg_k[0] = kp; L.n_alloc = na;
    L.n_true = N; L.k_true = K;
    std::unique_ptr<TmpBuf> w3buf, w2buf;
    TmpBuf flag(sizeof(int));
    if (g_knobs.gemm_variant == 3 || g_knobs.gemm_variant == 5) {   // split variants: limb images via a host round trip (test path only)
        FC_HIP(hipStreamSynchronize(s));
        std::vector<float> hw((size_t)na * kp);
        FC_HIP(hipMemcpy(hw.data(), wp.f(), hw.size() * 4, hipMemcpyDeviceToHost));
        const std::vector<unsigned short> w3 = make_bf16_limbs(hw, na, kp);
        w3buf.reset(new TmpBuf(w3.size() * 2));
        FC_HIP(hipMemcpy(w3buf->p, w3.data(), w3.size() * 2, hipMemcpyHostToDevice));
        L.W3 = (unsigned short*)w3buf->p;
        const std::vector<unsigned short> w2 = make_f16_limbs(hw, na, kp);
        if (!w2.empty()) {
            w2buf.reset(new TmpBuf(w2.size() * 2));
            FC_HIP(hipMemcpy(w2buf->p, w2.data(), w2.size() * 2, hipMemcpyHostToDevice));
            L.W2 = (unsigned short*)w2buf->p;
        }
    }
    GemmEpi e{};
    e.act = act; e.C = cp.f(); e.ldc = np;
    if (residual) { e.residual = rpad.f(); e.ldr = np; }
    ASeg a{xp.f(), kp};
    run_fp16_guarded((int*)flag.p, s, [&] { launch_gemm(L, &a, rp, e, EPI_LINEAR, s); });
    launch_pack_rows(cp.f(), np, N, y, N, 0, N, rows, s);
    FC_HIP(hipStreamSynchronize(s));
    FC_API_END
}

/* in_layer + hidden layers of one reference MLP (models/nets.py:19-30) at hidden width 512 over cat(x0, x1) (+ the rank-1 extra-context
   term rowscal[row] * net.colvec): the last hidden activation, decoded from the limb image the output GEMM would consume.  use_rows 1:
   the row-resident chain kernel (mlprows.hip); 0: one GEMM launch per layer (limb-chained); any other value is FC_ERR_INVALID.  Tensors (host fp32): net.in_layer.{weight,bias},
   net.layers.i.{weight,bias}, net.out_layer.weight (shape check only), optional net.colvec [512]. */
int fc_op_mlp_hidden_f32(const float* x0, int32_t k0, const float* x1, int32_t k1, const float* rowscal, const fc_tensor* tensors, int32_t n_tensors,
                         float* out, int32_t rows, int32_t act, int32_t use_rows, void* stream) {
    FC_API_BEGIN
    using namespace fc;
    if (!x0 || !out || rows < 1 || k0 < 1 || k1 < 0 || (k1 > 0 && !x1)) throw Error(FC_ERR_INVALID, "fc_op_mlp_hidden_f32: bad argument");
    if (use_rows != 0 && use_rows != 1) throw Error(FC_ERR_INVALID, "fc_op_mlp_hidden_f32: use_rows must be 0 (one GEMM launch per layer) or 1 (the row-resident chain kernel)");
    hipStream_t s = (hipStream_t)stream;
    WeightTable wt(tensors, n_tensors);
    DeviceArena arena;
    PackedMLP m;
    pack_mlp_mid(arena, wt, "net", m);
    const int H = m.sizes[0], p0 = round_up(k0, 32), p1 = k1 > 0 ? round_up(k1, 32) : 0;
    for (int h : m.sizes) if (h != 512) throw Error(FC_ERR_UNSUPPORTED, "fc_op_mlp_hidden_f32: hidden width must be 512");
    {
        const HostTensor& w = wt.get("net.in_layer.weight", {H, k0 + k1});
        std::vector<int> km = map_prefix(k0, p0);
        for (int j = 0; j < p1; ++j) km.push_back(j < k1 ? k0 + j : -1);
        VecD cv;
        if (wt.has("net.colvec")) cv = vec_from(wt.get("net.colvec", {H}));
        std::vector<int> segk = {p0};
        if (p1) segk.push_back(p1);
        m.in_layer = pack_linear(arena, mat_from(w), vec_from(wt.get("net.in_layer.bias", {H})), cv, map_prefix(H, H), km, segk);
    }
    attach_mlp_rows_images(arena, m);
    const int rp = round_up(rows, ROW_PAD);
    TmpBuf xa((size_t)rp * p0 * 4), xb((size_t)rp * std::max(p1, 32) * 4), h0((size_t)rp * 512 * 4), h1((size_t)rp * 512 * 4), h2((size_t)rp * 512 * 4),
        h16((size_t)rp * 512 * 4), flag(sizeof(int)), rs((size_t)rp * 4);
    launch_fill(xa.f(), 0.f, (size_t)rp * p0, s);
    launch_fill(xb.f(), 0.f, (size_t)rp * std::max(p1, 32), s);
    launch_fill(rs.f(), 0.f, (size_t)rp, s);
    launch_pack_rows(x0, k0, k0, xa.f(), p0, 0, k0, rows, s);
    if (k1 > 0) launch_pack_rows(x1, k1, k1, xb.f(), p1, 0, k1, rows, s);
    if (rowscal) launch_pack_rows(rowscal, 1, 1, rs.f(), 1, 0, 1, rows, s);
    float* const h[3] = {h0.f(), h1.f(), h2.f()};
    ASeg segs[2] = {{xa.f(), p0}, {xb.f(), std::max(p1, 32)}};
    const float* rsp = rowscal && m.in_layer.colvec ? rs.f() : nullptr;
    FC_HIP(hipDeviceSynchronize());                       // (the images were built on the null stream)
    run_fp16_guarded((int*)flag.p, s, [&] {
        if (use_rows == 1) launch_mlp_rows(m.in_layer, m.mid, segs, rsp, act, h, (unsigned short*)h16.p, rp, rows, s);
        else if (run_mlp_hidden_generic(m, segs, rsp, act, h, 512, rp, s, rows, (unsigned short*)h16.p, 0.f) != -1)
            throw Error(FC_ERR_INVALID, "fc_op_mlp_hidden_f32: the limb chain is off");
    });
    launch_limb_decode((const unsigned short*)h16.p, out, 512, rows, 512, s);
    FC_HIP(hipStreamSynchronize(s));
    FC_API_END
}

/* diagnostic / test entry (not part of fcflow.h): the query side of ONE attention pre-conditioner by itself (models/cif_block.py:14-20, models/perceiver.py:18-35,
   104-106): q [rows, I] = LayerNorm(mlp(x)) Wq^T I^-0.5 log2 e, packed by the engine's own code (pack_mlp_mid, pack_plain_linear, fold_q_projection /
   pack_q_projection / build_lnq of flow_pack.cpp; no K|V fold) and run on the path asked for:
     path 0  the row-resident kernel premlp_rows_kernel (premlp.hip), or FC_ERR_UNSUPPORTED where the engine's own conditions for it (premlp_fusable,
             premlp_rows_ok, with a pre-layer premlp_lu_fusable) do not hold -- never another path
     path 1  separate hidden-layer launches, then out_layer + LayerNorm + q as ONE GEMM (EPI_LNQ) and launch_lnq_finalize
     path 2  separate hidden layers, out_layer, launch_layernorm, q GEMM
   The repeat after a raised range flag takes path 2 on the bf16 limbs, as the engine's does.
   x [rows, ldx] (device): the in_layer reads its first k_in columns; columns k_in .. min(ldx, K_pad) - 1 reach the staged panel as they are (the
   engine's latent has the first x2 columns there; the packed weights are zero in them), everything beyond and the pad rows are zeros.
   Tensors (host fp32): net.in_layer.*, net.layers.<i>.*, net.out_layer.*, norm.{weight,bias}, to_q.weight [I, A_in]; optionally the previous flow
   layer's folded ActNorm + permuter lu.weight [D, D], lu.bias [D], packed as BlockPack::lin: then xprev [rows, D] is read instead of x (k_in = D / 2),
   xnext [rows, D] = lu(xprev) is written, and path 0 runs the map as the kernel's pre-layer (the other paths: as its own GEMM first). */
int fc_debug_premlp_q_f32(const float* x, int32_t ldx, int32_t k_in, const fc_tensor* tensors, int32_t n_tensors, const float* xprev, int32_t D,
                          float* xnext, float* q, int32_t rows, int32_t act, int32_t path, void* stream) {
    FC_API_BEGIN
    using namespace fc;
    const std::string who = "fc_debug_premlp_q_f32: ";
    if (!q || rows < 1 || k_in < 1) throw Error(FC_ERR_INVALID, who + "bad argument");
    if (path < 0 || path > 2) throw Error(FC_ERR_INVALID, who + "path must be 0 (the row-resident kernel), 1 (LayerNorm -> q fold GEMM) or 2 (separate launches)");
    if (act < FC_ACT_NONE || act > FC_ACT_LRELU02) throw Error(FC_ERR_INVALID, who + "unknown activation code");
    hipStream_t s = (hipStream_t)stream;
    WeightTable wt(tensors, n_tensors);
    const bool pre = wt.has("lu.weight");
    if (pre ? (!xprev || !xnext || D < 2) : (!x || ldx < k_in)) throw Error(FC_ERR_INVALID, who + (pre ? "a pre-layer needs xprev, xnext and D" : "x must have at least k_in columns"));
    DeviceArena arena;
    PackedMLP m;
    AttnPack at;
    Dims d{};
    {
        MatD wq;
        VecD bq;
        fold_q_projection(wt, "to_q", "norm", wq, bq);
        d.I = wq.rows; d.I_pad = pad_inner(d.I); d.A_in = wq.cols; d.A_in_pad = round_up(d.A_in, 32);
        pack_q_projection(arena, wq, bq, d, at);
    }
    pack_mlp_mid(arena, wt, "net", m);
    const int kp = round_up(k_in, 32);
    m.in_layer = pack_plain_linear(arena, wt, "net.in_layer", k_in, kp);
    m.out_layer = pack_plain_linear(arena, wt, "net.out_layer", m.sizes.back(), round_up(m.sizes.back(), 32));
    if (m.out_layer.N_pad != d.A_in_pad) throw Error(FC_ERR_SHAPE, who + "net.out_layer's output width != to_q's input width");
    build_lnq(arena, d, wt, "net.out_layer", at);
    // the pre-layer in the latent's padded layout [x1 | 0-pad | x2 | 0-pad] (flow_pack.cpp build_lin)
    PackedLinear lu;
    const int d1 = pre ? D / 2 : 0, d2 = D - d1, d1p = round_up(d1, 32), d2p = round_up(d2, 32), ldl = d1p + d2p;
    if (pre) {
        if (k_in != d1) throw Error(FC_ERR_INVALID, who + "with a pre-layer the in_layer reads x1, the first D / 2 latent dims");
        const std::vector<int> xl = map_xlayout(d1, d1p, d2, d2p);
        lu = pack_linear(arena, mat_from(wt.get("lu.weight", {D, D})), vec_from(wt.get("lu.bias", {D})), {}, xl, xl, {ldl});
    }
    const int rp = round_up(rows, ROW_PAD), lda = pre ? ldl : kp, ldh = std::max({max_hidden_pad(m), d.A_in_pad, 32});
    const size_t nh = (size_t)rp * ldh;
    TmpBuf xa((size_t)rp * lda * 4), xp(pre ? (size_t)rp * ldl * 4 : 4), h0(nh * 4), h1(nh * 4), h2(nh * 4), qb((size_t)rp * d.I_pad * 4),
        lnss((size_t)rp * (d.A_in_pad / 64 + 1) * 4), flag(sizeof(int));
    launch_fill(xa.f(), 0.f, (size_t)rp * lda, s);
    if (pre) {
        launch_fill(xp.f(), 0.f, (size_t)rp * ldl, s);
        launch_pack_rows(xprev, D, d1, xp.f(), ldl, 0, d1, rows, s);
        launch_pack_rows(xprev + d1, D, d2, xp.f(), ldl, d1p, d2, rows, s);
    } else {
        const int carried = std::min((int)ldx, kp);
        launch_pack_rows(x, ldx, carried, xa.f(), kp, 0, carried, rows, s);
    }
    float* const h[3] = {h0.f(), h1.f(), h2.f()};
    FC_HIP(hipDeviceSynchronize());                       // (the images were built on the null stream)
    int pass = 0;
    run_fp16_guarded((int*)flag.p, s, [&] {
        const int pth = pass++ > 0 ? 2 : path;            // the repeat after a raised range flag: separate launches on the bf16 limbs
        const ASeg in{xa.f(), lda};
        if (pth == 0) {
            const bool fusable = premlp_fusable(m.in_layer, m.mid, m.out_layer, at.q), rows_ok = premlp_rows_ok(rp, d.I_pad, qb.f(), h0.f(), nh),
                       lu_ok = pre && premlp_lu_fusable(lu, m.in_layer, act, lda);
            if (!fusable || lda < m.in_layer.K_pad || !rows_ok || (pre && !lu_ok))
                throw Error(FC_ERR_UNSUPPORTED, who + "path 0 asks for the row-resident kernel, which does not take this chain: " +
                                                premlp_refusal(m, at, d, fusable, rows_ok, pre, lu_ok, lu, act, D));
            launch_premlp(xa.f(), lda, m.in_layer, m.mid, m.out_layer, at.q, act, qb.f(), d.I_pad, rp, rows, s, h0.f(), nh, pre ? &lu : nullptr,
                          pre ? xp.f() : nullptr);
            return;
        }
        if (pre) {
            const ASeg ax{xp.f(), ldl};
            GemmEpi e{};
            e.C = xa.f(); e.ldc = ldl; e.rows_valid = rows;
            launch_gemm(lu, &ax, rp, e, EPI_LINEAR, s);
        }
        const int cur = run_mlp_hidden_generic(m, &in, nullptr, act, h, ldh, rp, s, rows);
        const ASeg a{h[cur], ldh};
        if (pth == 1) {
            if (!at.has_lnq || !gemm_lnq_ok())
                throw Error(FC_ERR_UNSUPPORTED, who + "path 1 asks for the LayerNorm -> q fold GEMM, which does not take this chain (build_lnq's shapes, lnq_fold (knob 10), a split-fp16 guard scope)");
            GemmEpi e{};
            e.C = qb.f(); e.ldc = d.I_pad; e.d2 = d.A_in; e.ldj_part = lnss.f(); e.ldj_pitch = (size_t)rp; e.rows_valid = rows;
            launch_gemm(at.lnq, &a, rp, e, EPI_LNQ, s);
            launch_lnq_finalize(qb.f(), d.I_pad, lnss.f(), d.A_in / 64, (size_t)rp, d.A_in, at.q_bias, rows, s);
            return;
        }
        int o = 0;
        while (o == cur) ++o;
        GemmEpi e{};
        e.C = h[o]; e.ldc = ldh; e.rows_valid = rows;
        launch_gemm(m.out_layer, &a, rp, e, EPI_LINEAR, s);
        launch_layernorm(h[o], ldh, d.A_in, rows, s);
        const ASeg aq{h[o], ldh};
        GemmEpi eq{};
        eq.C = qb.f(); eq.ldc = d.I_pad; eq.rows_valid = rows;
        launch_gemm(at.q, &aq, rp, eq, EPI_LINEAR, s);
    });
    launch_pack_rows(qb.f(), d.I_pad, d.I, q, d.I, 0, d.I, rows, s);
    if (pre) {
        launch_pack_rows(xa.f(), ldl, d1, xnext, D, 0, d1, rows, s);
        launch_pack_rows(xa.f() + d1p, ldl, d2, xnext, D, d1, d2, rows, s);
    }
    FC_HIP(hipStreamSynchronize(s));
    FC_API_END
}

// fc_op_attention_f32 / fc_debug_attention_ctx_f32 and their namesakes with per-scene key counts (fcflow_context_counts.h) share one body each.
// With counts the key / value tensors are copied and the copies' pad rows zeroed first -- what the flow engine does to its context panel -- so
// that what a caller left in pad rows reaches no limb image and no range flag.
namespace fc {
struct CountedCopy {
    std::unique_ptr<TmpBuf> buf;
    // src [B][M][D] as it is (null counts), or a copy whose rows >= clamp(counts[b], 1, M) are zeros
    const float* of(const char* who, const float* src, const int32_t* counts, int B, int M, int D, hipStream_t s) {
        if (!counts) return src;
        if (B < 1 || M < 1) throw Error(FC_ERR_INVALID, std::string(who) + ": B, N, M must be positive");
        const size_t bytes = (size_t)B * M * D * sizeof(float);
        buf.reset(new TmpBuf(bytes));
        FC_HIP(hipMemcpyAsync(buf->p, src, bytes, hipMemcpyDeviceToDevice, s));
        launch_zero_pad_rows(buf->f(), D, counts, B, M, s);
        return buf->f();
    }
};

static void op_attention(const char* who_c, bool counted, const float* q, const float* k, const float* v, float* out, const int32_t* counts, int B, int N, int M,
                         int D, float scale, hipStream_t s) {
    const std::string who = who_c;
    if (!q || !k || !v || !out || (counted && !counts)) throw Error(FC_ERR_INVALID, who + ": null pointer");
    if (D != 32 && D != 64 && D != 128 && D != 256) throw Error(FC_ERR_UNSUPPORTED, who + ": D must be 32, 64 or 128, or 256");
    CountedCopy kc, vc;
    k = kc.of(who_c, k, counts, B, M, D, s);
    v = vc.of(who_c, v, counts, B, M, D, s);
    TmpBuf limbs(attention_limb_ws_bytes((long)B * M, D)), flag(sizeof(int));
    run_fp16_guarded((int*)flag.p, s, [&] { launch_attention({q, D, scale * kLog2eF}, AttnKeys::panels(k, D, v, D, limbs.p), {B, N, N, M, M, D, counts}, out, D, s); });
    FC_HIP(hipStreamSynchronize(s));
}

static void op_attention_ctx(const char* who_c, bool counted, const float* q, const float* c, float* out, const int32_t* counts, int B, int N, int M, int D,
                             float scale, hipStream_t s) {
    const std::string who = who_c;
    if (!q || !c || !out || (counted && !counts)) throw Error(FC_ERR_INVALID, who + ": null pointer");
    if (D != 32 && D != 64) throw Error(FC_ERR_UNSUPPORTED, who + ": D must be 32 or 64");
    if (((uintptr_t)q | (uintptr_t)c | (uintptr_t)out) & 15) throw Error(FC_ERR_INVALID, who + ": operands must be 16-byte aligned");
    CountedCopy cc;
    c = cc.of(who_c, c, counts, B, M, D, s);
    TmpBuf limbs(attention_limb_ws_bytes((long)B * M, D) / 2), flag(sizeof(int));
    run_fp16_guarded((int*)flag.p, s, [&] {
        if (gemm_fp16_flag() && g_knobs.attn_fp16) {
            launch_context_limbs(c, D, (unsigned short*)limbs.p, (long)B * M, D, s);
            launch_attention({q, D, scale * kLog2eF}, AttnKeys::context((const unsigned short*)limbs.p), {B, N, N, M, M, D, counts}, out, D, s);
        } else {                                        // as in the engine: the repeat after a raised range flag (and attn_fp16, knob 5, = 0) takes c itself, in fp32
            launch_attention({q, D, scale * kLog2eF}, AttnKeys::panels(c, D, c, D, nullptr), {B, N, N, M, M, D, counts}, out, D, s);
        }
    });
    FC_HIP(hipStreamSynchronize(s));
}
}  // namespace fc

int fc_op_attention_f32(const float* q, const float* k, const float* v, float* out, int32_t B, int32_t N, int32_t M, int32_t D, float scale,
                        void* stream) {
    FC_API_BEGIN
    fc::op_attention("fc_op_attention_f32", false, q, k, v, out, nullptr, B, N, M, D, scale, (hipStream_t)stream);
    FC_API_END
}

int fc_op_attention_counts_f32(const float* q, const float* k, const float* v, float* out, const int32_t* ctx_counts, int32_t B, int32_t N, int32_t M,
                               int32_t D, float scale, void* stream) {
    FC_API_BEGIN
    fc::op_attention("fc_op_attention_counts_f32", true, q, k, v, out, ctx_counts, B, N, M, D, scale, (hipStream_t)stream);
    FC_API_END
}

/* out[B,N,D] = softmax(q c^T * scale) c with ONE tensor c [B,M,D] as keys and values, on the kernels of the folded flow engine (to_kv folded
   away, flow_engine.cpp): one limb image of c, then attn16_kernel<64, 1> (D = 64: one staged tile per 64 keys) or attn16_kernel<32> on that
   image twice.  For the tests; a value beyond the image's range is an error here (the engine repeats such a pass on its fp32 path). */
int fc_debug_attention_ctx_f32(const float* q, const float* c, float* out, int32_t B, int32_t N, int32_t M, int32_t D, float scale, void* stream) {
    FC_API_BEGIN
    fc::op_attention_ctx("fc_debug_attention_ctx_f32", false, q, c, out, nullptr, B, N, M, D, scale, (hipStream_t)stream);
    FC_API_END
}

/* the same with per-scene key counts, declared in fcflow_context_counts.h */
int fc_op_attention_ctx_counts_f32(const float* q, const float* c, float* out, const int32_t* ctx_counts, int32_t B, int32_t N, int32_t M, int32_t D,
                                   float scale, void* stream) {
    FC_API_BEGIN
    fc::op_attention_ctx("fc_op_attention_ctx_counts_f32", true, q, c, out, ctx_counts, B, N, M, D, scale, (hipStream_t)stream);
    FC_API_END
}

int fc_op_attention_weights_f32(const float* q, const float* k, float* out, const int32_t* sel, int32_t P, int32_t sel_per_scene,
                                int32_t B, int32_t N, int32_t M, int32_t D, float scale, void* stream) {
    FC_API_BEGIN
    if (!q || !k || !out) throw fc::Error(FC_ERR_INVALID, "fc_op_attention_weights_f32: null pointer");
    if (D != 32 && D != 64 && D != 128 && D != 256) throw fc::Error(FC_ERR_UNSUPPORTED, "fc_op_attention_weights_f32: D must be 32, 64 or 128, or 256");
    fc::launch_attention_weights({q, D, scale * fc::kLog2eF}, fc::AttnKeys::panels(k, D, nullptr, 0, nullptr), {B, N, N, M, M, D}, sel, sel ? P : N, sel_per_scene, out,
                                 (hipStream_t)stream);
    FC_HIP(hipStreamSynchronize((hipStream_t)stream));
    FC_API_END
}

size_t fc_op_attention_mass_scratch_bytes(int32_t B, int32_t N, int32_t M) { return B < 1 || N < 1 || M < 1 ? 0 : fc::attention_mass_slab_bytes(B, N, M); }

int fc_op_attention_mass_f32(const float* q, const float* k, const float* row_weight, float* out, int32_t B, int32_t N, int32_t M, int32_t D, float scale,
                             void* scratch, size_t scratch_bytes, void* stream) {
    FC_API_BEGIN
    if (!q || !k || !out || !scratch) throw fc::Error(FC_ERR_INVALID, "fc_op_attention_mass_f32: null pointer");
    if (B < 1 || N < 1 || M < 1) throw fc::Error(FC_ERR_INVALID, "fc_op_attention_mass_f32: B, N, M must be positive");
    if (D != 32 && D != 64 && D != 128 && D != 256) throw fc::Error(FC_ERR_UNSUPPORTED, "fc_op_attention_mass_f32: D must be 32, 64, 128 or 256");
    if (scratch_bytes < fc::attention_mass_slab_bytes(B, N, M))
        throw fc::Error(FC_ERR_WORKSPACE, "fc_op_attention_mass_f32: scratch too small: " + std::to_string(scratch_bytes) + " bytes given, " +
                                          std::to_string(fc::attention_mass_slab_bytes(B, N, M)) + " needed (fc_op_attention_mass_scratch_bytes)");
    if ((uintptr_t)scratch & 15) throw fc::Error(FC_ERR_INVALID, "fc_op_attention_mass_f32: scratch must be 16-byte aligned");
    fc::launch_attention_mass({q, D, scale * fc::kLog2eF}, fc::AttnKeys::panels(k, D, nullptr, 0, nullptr), {B, N, N, M, M, D}, row_weight, (float*)scratch, out,
                              (hipStream_t)stream);
    FC_HIP(hipStreamSynchronize((hipStream_t)stream));
    FC_API_END
}

int fc_op_knn_f32(const float* f, int32_t* idx, int32_t B, int32_t M, int32_t C, int32_t k, void* stream) {
    FC_API_BEGIN
    using namespace fc;
    if (!f || !idx || B < 1 || M < 1 || C < 1) throw Error(FC_ERR_INVALID, "fc_op_knn_f32: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int cp = round_up(C, 32);
    knn_check_shape(cp, C, M, k);
    TmpBuf fp((size_t)B * M * cp * 4);
    launch_pack_rows(f, C, C, fp.f(), cp, 0, cp, B * M, s);
    launch_knn(fp.f(), cp, C, idx, B, M, M, k, s);
    FC_HIP(hipStreamSynchronize(s));
    FC_API_END
}

// the same search started from given neighbour sets (what the DGCNN engine does between its levels): idx_warm [B, M, k] int32, may equal idx
int fc_op_knn_warm_f32(const float* f, const int32_t* idx_warm, int32_t* idx, int32_t B, int32_t M, int32_t C, int32_t k, void* stream) {
    FC_API_BEGIN
    using namespace fc;
    if (!f || !idx || !idx_warm || B < 1 || M < 1 || C < 1) throw Error(FC_ERR_INVALID, "fc_op_knn_warm_f32: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int cp = round_up(C, 32);
    knn_check_shape(cp, C, M, k);
    TmpBuf fp((size_t)B * M * cp * 4);
    launch_pack_rows(f, C, C, fp.f(), cp, 0, cp, B * M, s);
    launch_knn(fp.f(), cp, C, idx, B, M, M, k, s, idx_warm);
    FC_HIP(hipStreamSynchronize(s));
    FC_API_END
}

// the search with per-scene point counts (fcflow_embed_counts.h): idx_warm null = cold; rows >= a scene's count of idx are left as they are
int fc_op_knn_counts_f32(const float* f, const int32_t* idx_warm, const int32_t* counts, int32_t count_min, int32_t count_max, int32_t* idx, int32_t B, int32_t M,
                         int32_t C, int32_t k, void* stream) {
    FC_API_BEGIN
    using namespace fc;
    if (!f || !idx || B < 1 || M < 1 || C < 1) throw Error(FC_ERR_INVALID, "fc_op_knn_counts_f32: bad argument");
    if (!counts) throw Error(FC_ERR_INVALID, "fc_op_knn_counts_f32: null counts (the search without counts is fc_op_knn_f32)");
    hipStream_t s = (hipStream_t)stream;
    const int cp = round_up(C, 32);
    const SceneCounts cnt{counts, count_min, count_max};
    knn_check_counts(cp, C, M, k, cnt);
    TmpBuf fp((size_t)B * M * cp * 4);
    launch_pack_rows(f, C, C, fp.f(), cp, 0, cp, B * M, s);
    launch_knn_counts(fp.f(), cp, C, idx, B, M, M, k, s, idx_warm, cnt);
    FC_HIP(hipStreamSynchronize(s));
    FC_API_END
}

int fc_op_fps_f32(const float* xyz, int32_t* idx, int32_t B, int32_t n, int32_t m, void* stream) {
    FC_API_BEGIN
    if (!xyz || !idx || B < 1 || n < 1 || m < 0) throw fc::Error(FC_ERR_INVALID, "fc_op_fps_f32: bad argument");
    /* (single-operator entry of the test / training paths: the one scratch array of the > 8192-point variant is allocated here, stream-ordered;
     * the engine's own calls carve it from the caller's workspace) */
    float* scratch = nullptr;
    const size_t nf = fc::fps_scratch_floats(B, n);
    if (nf) FC_HIP(hipMallocAsync((void**)&scratch, nf * sizeof(float), (hipStream_t)stream));
    try { fc::launch_fps(xyz, 3, idx, B, n, m, scratch, (hipStream_t)stream); }
    catch (...) { if (scratch) (void)hipFreeAsync(scratch, (hipStream_t)stream); throw; }
    if (scratch) FC_HIP(hipFreeAsync(scratch, (hipStream_t)stream));
    FC_API_END
}

int fc_stage_fps_f32(const float* pts, int32_t ld, int32_t C, int64_t* idx, int32_t B, int32_t n, int32_t m, void* stream) {
    FC_API_BEGIN
    if (!pts || !idx || B < 1 || n < 1 || m < 1) throw fc::Error(FC_ERR_INVALID, "fc_stage_fps_f32: bad argument");
    fc::TmpBuf scratch(n > 24576 ? (size_t)B * n * sizeof(float) : 4);
    fc::launch_fps_nd(pts, ld, C, idx, B, n, m, scratch.f(), (hipStream_t)stream);
    FC_HIP(hipStreamSynchronize((hipStream_t)stream));
    FC_API_END
}

int fc_stage_co_unit_sphere_f32(const float* p0, int32_t n0, const float* p1, int32_t n1, int32_t ld, float* out0, float* out1, float* inverse,
                                int32_t B, void* stream) {
    FC_API_BEGIN
    if (!p0 || !out0 || !inverse || (n1 > 0 && (!p1 || !out1))) throw fc::Error(FC_ERR_INVALID, "fc_stage_co_unit_sphere_f32: null pointer");
    fc::launch_co_unit_sphere(p0, n0, n1 > 0 ? p1 : p0, n1, ld, out0, n1 > 0 ? out1 : out0, inverse, B, (hipStream_t)stream);
    FC_API_END
}

int fc_clamp_infs_f32(float* t, int64_t n, void* stream) {
    FC_API_BEGIN
    if (!t || n < 0) throw fc::Error(FC_ERR_INVALID, "fc_clamp_infs_f32: bad argument");
    fc::TmpBuf tmp(4 * sizeof(float) + sizeof(int));
    fc::launch_clamp_infs(t, (long)n, tmp.f(), (int*)(tmp.f() + 4), (hipStream_t)stream);
    FC_HIP(hipStreamSynchronize((hipStream_t)stream));
    FC_API_END
}

int fc_change_map_f32(float* lp10, int32_t N, float* lp00, int32_t N0, float* out, int32_t B, float multiple, float hard_cutoff,
                      int32_t use_cutoff, int32_t* invalid, void* stream) {
    FC_API_BEGIN
    if (!lp10 || !lp00 || !out || !invalid) throw fc::Error(FC_ERR_INVALID, "fc_change_map_f32: null pointer");
    fc::TmpBuf tmp(4 * sizeof(float) + sizeof(int));
    int* status = (int*)(tmp.f() + 4);
    fc::launch_change_map(lp10, N, lp00, N0, out, B, multiple, hard_cutoff, use_cutoff, tmp.f(), status, (hipStream_t)stream);
    int h = 0;
    FC_HIP(hipMemcpyAsync(&h, status, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    FC_HIP(hipStreamSynchronize((hipStream_t)stream));
    *invalid = h;
    FC_API_END
}

int fc_change_map_ragged_f32(float* lp10, const int64_t* offsets, float* lp00, int32_t N0, float* out, int32_t B, float multiple, float hard_cutoff,
                             int32_t use_cutoff, int32_t* invalid, void* stream) {
    FC_API_BEGIN
    if (!lp10 || !offsets || !lp00 || !out || !invalid) throw fc::Error(FC_ERR_INVALID, "fc_change_map_ragged_f32: null pointer");
    fc::TmpBuf tmp(4 * sizeof(float) + sizeof(int));
    int* status = (int*)(tmp.f() + 4);
    fc::launch_change_map_ragged(lp10, offsets, lp00, N0, out, B, multiple, hard_cutoff, use_cutoff, tmp.f(), status, (hipStream_t)stream);
    int h = 0;
    FC_HIP(hipMemcpyAsync(&h, status, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    FC_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (h & 2) throw fc::Error(FC_ERR_INVALID, "fc_change_map_ragged_f32: offsets are not an ascending prefix sum of row counts below 2^31");
    *invalid = h & 1;
    FC_API_END
}

/* include/fcflow_sparse_target.h */
int fc_change_map_counts_f32(float* lp10, int32_t N, const int32_t* counts_1, float* lp00, int32_t N0, const int32_t* counts_0, float* out, int32_t B,
                             float multiple, float hard_cutoff, int32_t use_cutoff, int32_t* invalid, void* stream) {
    FC_API_BEGIN
    if (!lp10 || !counts_1 || !lp00 || !out || !invalid) throw fc::Error(FC_ERR_INVALID, "fc_change_map_counts_f32: null pointer");
    fc::TmpBuf tmp(4 * sizeof(float) + sizeof(int));
    int* status = (int*)(tmp.f() + 4);
    fc::launch_change_map_counts(lp10, N, counts_1, lp00, N0, counts_0, out, B, multiple, hard_cutoff, use_cutoff, tmp.f(), status, (hipStream_t)stream);
    int h = 0;
    FC_HIP(hipMemcpyAsync(&h, status, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    FC_HIP(hipStreamSynchronize((hipStream_t)stream));
    *invalid = h & 5;                                            /* bit 0: a result is not finite; bit 2: a baseline row shorter than 2 */
    FC_API_END
}

int fc_change_map_ragged_counts_f32(float* lp10, const int64_t* offsets, float* lp00, int32_t N0, const int32_t* counts_0, float* out, int32_t B,
                                    float multiple, float hard_cutoff, int32_t use_cutoff, int32_t* invalid, void* stream) {
    FC_API_BEGIN
    if (!lp10 || !offsets || !lp00 || !out || !invalid) throw fc::Error(FC_ERR_INVALID, "fc_change_map_ragged_counts_f32: null pointer");
    fc::TmpBuf tmp(4 * sizeof(float) + sizeof(int));
    int* status = (int*)(tmp.f() + 4);
    fc::launch_change_map_ragged_counts(lp10, offsets, lp00, N0, counts_0, out, B, multiple, hard_cutoff, use_cutoff, tmp.f(), status, (hipStream_t)stream);
    int h = 0;
    FC_HIP(hipMemcpyAsync(&h, status, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    FC_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (h & 2) throw fc::Error(FC_ERR_INVALID, "fc_change_map_ragged_counts_f32: offsets are not an ascending prefix sum of row counts below 2^31");
    *invalid = h & 5;
    FC_API_END
}

int fc_op_expm_action_f32(const float* params, int32_t ldp, const float* x2, int32_t ldx, const float* scal4, float* y2, int32_t ldy, float* ldj,
                          float* info, int32_t rows, int32_t d2, int32_t inverse, void* stream) {
    FC_API_BEGIN
    if (!params || !x2 || !scal4 || !y2 || rows < 1 || d2 < 1 || ldx < d2 || ldy < d2) throw fc::Error(FC_ERR_INVALID, "fc_op_expm_action_f32: bad argument");
    if (d2 <= fc::kExpmSmallMaxD2) throw fc::Error(FC_ERR_INVALID, "fc_op_expm_action_f32: d2 <= 16 runs on the one-lane-per-point kernel of the engine");
    fc::TmpBuf tmp(sizeof(int));
    int* status = (int*)tmp.p;
    hipStream_t s = (hipStream_t)stream;
    FC_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
    fc::launch_expm_wide(params, ldp, x2, ldx, scal4, y2, ldy, d2, ldj, ldj ? 1 : 0, rows, d2, inverse, status, info, s);
    int h = 0;
    FC_HIP(hipMemcpyAsync(&h, status, sizeof(int), hipMemcpyDeviceToHost, s));
    FC_HIP(hipStreamSynchronize(s));
    if (h) throw fc::Error(FC_ERR_UNSUPPORTED, "ExponentialCoupling: a coupling matrix norm ||W - mu I||_1 exceeds the matrix-exponential kernel's bound "
                                               "(40 Taylor steps, 534): the result would be a truncated series");
    FC_API_END
}

int fc_op_rqspline_f32(const float* x, const float* params, float* y, float* logabsdet, int64_t n, int32_t K, int32_t inverse, void* stream) {
    FC_API_BEGIN
    if (!x || !params || !y || !logabsdet || n < 0) throw fc::Error(FC_ERR_INVALID, "fc_op_rqspline_f32: bad argument");
    fc::launch_spline_flat(x, params, y, logabsdet, n, K, inverse, (hipStream_t)stream);
    FC_API_END
}

}  // extern "C"
