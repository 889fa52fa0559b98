"""fa.attention_weights / fc_flow_attention_weights_f32 / fc_op_attention_weights_f32 (csrc/attention_weights.hip) on the GPU: the softmax
rows the reference materialises as `attn_weights` (models/perceiver.py:108-115) and visualize_attention.py colours the context cloud with.

Gate everywhere a comparison with fp64 is made (attn_weights_util.gate):  max |w - w64| <= 4 x E,
E = max(max |w32 - w64|, 4 * 2^-24 * max w64), with w32 the same quantity from an fp32 evaluation that is NOT the code under test (torch
on the CPU, the reference's fp32 run in the fixture, the oracle in fp32).  Every test prints the measured ratio max |w - w64| / E."""

import numpy as np
import pytest
import torch

import attn_weights_util as U
import flowcompare_amd as fa
import knob_util
from conftest import Fixture
from flowcompare_amd import engine
from fullsize_util import build_conditioned, state_dicts, synth_pairs
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _kernels:
    """Names of the kernels launched inside the block (the in-library profiler's report): which path a call took is asserted, not assumed."""

    def __enter__(self):
        engine.profile_enable(True)
        engine.profile_reset()
        self.names = []
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                torch.cuda.synchronize()
                self.names = [r["kernel"] for r in engine.profile_report()]
        finally:
            engine.profile_enable(False)
            engine.profile_reset()
        return False

    def ran(self, substr):
        return any(substr in n for n in self.names)


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _ratio(label, w, w64, w32):
    """prints and returns max |w - w64| / E"""
    w, w64, w32 = (torch.as_tensor(t).double().cpu() for t in (w, w64, w32))
    err, e32, wmax = (w - w64).abs().max().item(), (w32 - w64).abs().max().item(), w64.max().item()
    bound = U.gate(e32, wmax)
    print(f"{label}: max |w - fp64| {err:.2e}   fp32 yardstick {e32:.2e}   max w {wmax:.3e}   ratio to E {4.0 * err / bound:.2f}  (gate 4)")
    return err, bound


# ------------------------------------------------------------------ 1. the operator against fp64
def _op_case(label, q, k, sm, points=None):
    s64 = (q.double() @ k.double().transpose(1, 2)) * sm
    w64 = torch.softmax(s64, -1)
    w32 = torch.softmax((q @ k.transpose(1, 2)) * sm, -1)            # the same formula in eager fp32 on the CPU
    w = engine.op_attention_weights(q.to(DEV), k.to(DEV), sm, points=points).cpu()
    if points is not None:
        idx = torch.as_tensor(points).long()
        w64, w32 = (t[:, idx] if idx.dim() == 1 else torch.stack([t[b, idx[b]] for b in range(t.shape[0])]) for t in (w64, w32))
    assert w.shape == w64.shape and w.dtype == torch.float32
    assert torch.isfinite(w).all() and (w >= 0).all()
    M = k.shape[1]
    assert (w.double().sum(-1) - 1.0).abs().max().item() <= M * 2.0 ** -23
    err, bound = _ratio(label, w, w64, w32)
    assert err <= bound, label


@pytest.mark.parametrize("B,N,M,D", [(2, 128, 64, 64), (3, 100, 130, 64), (1, 20, 24, 32), (2, 257, 1000, 64), (1, 64, 4096, 64), (2, 40, 70, 128),
                                     (2, 33, 1, 64), (1, 5, 1, 32), (2, 130, 1, 128), (1, 64, 16384, 64), (2, 300, 333, 128), (1, 129, 200, 32)])
def test_operator_matches_fp64(B, N, M, D):
    """The shapes of test_gpu_ops.test_attention_matches_fp64 (ragged N and M, one key tile, D = 32 / 64 / 128), M = 1 and M = 16 384."""
    q, k = _rand(B, N, D, seed=1, scale=2.0), _rand(B, M, D, seed=2, scale=2.0)
    _op_case(f"B {B} N {N} M {M} D {D}", q, k, D ** -0.5)


@pytest.mark.parametrize("B,N,M,D", [(2, 1024, 1000, 64), (1, 4096, 4096, 64), (3, 300, 777, 64), (2, 1000, 1250, 64), (1, 256, 64, 32), (2, 700, 33, 32)])
@pytest.mark.parametrize("scale", [1.0, 40.0, 0.05])
def test_operator_operand_scales(B, N, M, D, scale):
    """The shapes and the three operand scales of test_gpu_ops.test_attention_one_accumulator_form_against_fp64."""
    q, k = _rand(B, N, D, seed=51) * scale, _rand(B, M, D, seed=52) * scale
    _op_case(f"B {B} N {N} M {M} D {D} operand scale {scale}", q, k, 0.125 / (scale * scale))


@pytest.mark.parametrize("per_tile", [0.4, 1.5, 7.5])
def test_operator_score_ramps(per_tile):
    """Scores that rise along the key axis (test_gpu_ops.test_attention_lazy_reference_on_score_ramps): the running maximum of pass 1
    moves in every tile, and the last tiles hold all the weight."""
    B, N, M, D = 2, 200, 1024, 64
    q, k = _rand(B, N, D, seed=61), _rand(B, M, D, seed=62)
    q[..., 0] = 4.0
    k[..., 0] = torch.arange(M).float()[None, :] * (per_tile / 64.0 / (0.125 * 4.0))
    _op_case(f"ramp {per_tile} nats per tile", q, k, 0.125)


def test_operator_selection_forms():
    """points as [P] and [B, P], repeated and unsorted, on a ragged shape: the selected rows against fp64 and bit-equal to the full map's rows."""
    B, N, M, D = 3, 300, 777, 64
    q, k = _rand(B, N, D, seed=71, scale=2.0), _rand(B, M, D, seed=72, scale=2.0)
    full = engine.op_attention_weights(q.to(DEV), k.to(DEV), 0.125)
    shared = [299, 0, 17, 17, 128, 5]
    per = torch.tensor([[1, 1, 1, 298], [200, 3, 64, 0], [127, 128, 129, 127]])
    _op_case("points [P]", q, k, 0.125, points=shared)
    _op_case("points [B, P]", q, k, 0.125, points=per)
    assert torch.equal(engine.op_attention_weights(q.to(DEV), k.to(DEV), 0.125, points=shared), full[:, shared])
    got = engine.op_attention_weights(q.to(DEV), k.to(DEV), 0.125, points=per)
    assert torch.equal(got, torch.stack([full[b, per[b]] for b in range(B)]))
    big = torch.randint(0, N, (B, 200), generator=torch.Generator().manual_seed(5))       # more than one workgroup of selected rows
    got = engine.op_attention_weights(q.to(DEV), k.to(DEV), 0.125, points=big)
    assert torch.equal(got, torch.stack([full[b, big[b]] for b in range(B)]))


# ------------------------------------------------------------------ 2. the engine against the reference's weights
def _build(fx):
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    sd_flow, sd_emb = U.state_dicts(fx)
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    return cfg, md


def _fixture_inputs(fx):
    batch = tuple(None if t is None else t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
    return batch, [e.to(DEV) for e in fx.eps()]


def _check_fixture(case, label, cfg, md, fx, ref):
    batch, eps = _fixture_inputs(fx)
    layers = [U.layer_of(cfg, p) for p in ref.prefixes]
    ws = fa.attention_weights(batch, md, cfg, layers=layers, eps=eps)
    assert len(ws) == len(layers)
    worst = 0.0
    for i, w in enumerate(ws):
        assert tuple(w.shape) == ref.w64[i].shape and w.dtype == torch.float32
        err, bound = _ratio(f"{case} [{label}] attention {i} ({layers[i]})", w, ref.w64[i], ref.w32[i])
        worst = max(worst, err / bound)
    return worst


@pytest.mark.parametrize("case", list(U.CASES))
def test_engine_matches_reference_weights(case):
    """All attentions of each fixture against the reference's fp64 `attn_weights`, gated at 4 x E with both terms of E from the fixture
    (the reference's own fp32 run).  attnw_sharp_L3 is the one that matters (peaked rows); on the near-uniform ones a constant 1/M
    output would be 2 % off while the gate is ~1e-6 of the row maximum."""
    fx, ref = U.load_case(case)
    cfg, md = _build(fx)
    with _kernels() as kn:
        worst = _check_fixture(case, "default path", cfg, md, fx, ref)
    assert worst <= 1.0
    # real dims: head dim 64, K as the limb image; e2e_tiny_cif: head dim 32, limb image (4 attentions x 64 columns), three-launch q
    assert kn.ran("attn_weights_kernel<32, 1>" if case == "e2e_tiny_cif" else "attn_weights_kernel<64, 1>"), kn.names
    assert kn.ran("layernorm_kernel") == (case == "e2e_tiny_cif") and kn.ran("premlp_rows_kernel") == (case != "e2e_tiny_cif")


# ------------------------------------------------------------------ 3. exact properties
@pytest.mark.parametrize("case", [U.SHARP, "e2e_tiny_cif"])
def test_exact_properties(case):
    fx, ref = U.load_case(case)
    cfg, md = _build(fx)
    batch, eps = _fixture_inputs(fx)
    B, N, M = fx.meta["B"], fx.meta["N"], fx.meta["M"]
    layers = [U.layer_of(cfg, p) for p in ref.prefixes]
    _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    full, lp_w = fa.attention_weights(batch, md, cfg, layers=layers, eps=eps, return_log_prob=True)
    assert torch.equal(lp_w, lp), "the probe disturbed the pass"
    assert torch.equal(fa.inner_loop(batch, md, cfg, eps=eps)[1], lp)
    again = fa.attention_weights(batch, md, cfg, layers=layers, eps=eps)
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    for w in full:
        assert tuple(w.shape) == (B, N, M)                          # exactly M columns: 80 and 24 are not tile multiples
        assert torch.isfinite(w).all() and (w >= 0).all()
        assert (w.double().sum(-1) - 1.0).abs().max().item() <= M * 2.0 ** -23
    shared = [N - 1, 0, 3, 3, 1]
    per = torch.tensor([[2, 2, N - 1], [0, N - 2, 1]])
    got = fa.attention_weights(batch, md, cfg, layers=layers, points=shared, eps=eps)
    for w, f in zip(got, full):
        assert torch.equal(w, f[:, shared])
    got = fa.attention_weights(batch, md, cfg, layers=layers, points=per.to(DEV), eps=eps)
    for w, f in zip(got, full):
        assert torch.equal(w, torch.stack([f[b, per[b]] for b in range(B)]))
    for i, l in enumerate(layers):                                  # alone, and with the others in another order
        assert torch.equal(fa.attention_weights(batch, md, cfg, layers=(l,), eps=eps)[0], full[i])
    rev = fa.attention_weights(batch, md, cfg, layers=layers[::-1], eps=eps)
    for w, f in zip(rev, full[::-1]):
        assert torch.equal(w, f)
    # under the deferred range check the call only enqueues its pass; same bits once resolved
    with engine.deferred_range_check() as drc:
        dq, dlp = fa.attention_weights(batch, md, cfg, layers=layers, points=shared, eps=eps, return_log_prob=True)
    assert drc.repeated == 0 and torch.equal(dlp, lp)
    for w, f in zip(dq, full):
        assert torch.equal(w, f[:, shared])
    assert md["flow"].last_eps is not None
    drawn = fa.attention_weights(batch, md, cfg, layers=("aug",), points=[0])         # eps drawn like log_prob does
    assert tuple(drawn[0].shape) == (B, 1, M) and len(md["flow"].last_eps) == len(eps)


# ------------------------------------------------------------------ 4. operand forms
# (label, knobs, K form of the weight kernel, the kernels that mark the q forms of the run: premlp_rows = final from the row-resident chain,
#  lnq_finalize = finalised by that pass, layernorm = three-launch fallback; none of them = the LayerNorm -> q GEMM whose q the consumer
#  finishes on load).  The augmenter's 6-wide input never admits the row-resident chain: by default ITS q is the fold finished on load.
PATHS = [("row-resident chain q (augmenter: fold finished on load), limb-image K (default)", {}, 1, {"premlp_rows_kernel"}),
         ("LayerNorm -> q fold finished on load, limb-image K", {8: 0}, 1, set()),
         ("LayerNorm -> q fold + launch_lnq_finalize, fp32 K", {8: 0, 5: 0}, 0, {"lnq_finalize_kernel"}),
         ("three-launch fallback q, limb-image K", {8: 0, 10: 0}, 1, {"layernorm_kernel"}),
         ("row-resident chain q (augmenter: launch_lnq_finalize), fp32 K", {5: 0}, 0, {"premlp_rows_kernel", "lnq_finalize_kernel"}),
         ("no guard scope (bf16-limb GEMMs): three-launch q, fp32 K", {0: 3}, 0, {"layernorm_kernel"})]


@pytest.mark.parametrize("label,knobs,kform,qmarks", PATHS, ids=["default", "fold_on_load", "fold_finalize-fp32_K", "three_launch", "chain-fp32_K", "no_guard_scope"])
def test_every_operand_form_on_the_sharp_fixture(label, knobs, kform, qmarks):
    """Which run leaves q / K in which form (csrc/flow_engine.cpp attention_keys / run_attention, prepare), all at the real dims of attnw_sharp_L3 (head dim 64,
    pre-attention MLP 256 wide), selected with the fc_debug_set keys tests/test_gpu_flow.py uses and restored afterwards:
      q final from launch_premlp            default (knob 8 = 2), flow layers        K limb image: whenever knob 5 = 1 inside a guard scope
      q un-normalised, finished on load     default, the augmenter; knob 8 = 0: all  K fp32 panel: knob 5 = 0, knob 0 = 3 (no guard scope)
      q finalised by launch_lnq_finalize    knobs 8 = 0, 5 = 0; knob 5 = 0 (augmenter)
      q from the three-launch fallback      knobs 8 = 0, 10 = 0; knob 0 = 3
    Head dim 32 is covered by e2e_tiny_cif in test_engine_matches_reference_weights (three-launch q: A_in = 8 admits neither fused form;
    limb-image K: 4 attentions x 64 columns), head dim 32 with an fp32 K panel and head dim 128 by test_other_head_dims_against_the_oracle,
    the range-fallback pass by test_range_fallback_pass_rewrites_the_weights.  Same gate as the default path; the kernels that ran are read
    from the in-library profiler, so each form is known to have been produced."""
    fx, ref = U.load_case(U.SHARP)
    cfg, md = _build(fx)
    with _kernels() as kn, knob_util.knobs(knobs):
        worst = _check_fixture(U.SHARP, label, cfg, md, fx, ref)
    assert worst <= 1.0
    assert kn.ran(f"attn_weights_kernel<64, {kform}>") and not kn.ran(f"attn_weights_kernel<64, {1 - kform}>"), kn.names
    for mark in ("premlp_rows_kernel", "lnq_finalize_kernel", "layernorm_kernel"):
        assert kn.ran(mark) == (mark in qmarks), (mark, kn.names)


def _against_oracle(label, cfg, md, e0, e1, extra, eps, layers, points=None, scene=None):
    """HIP weights against the oracle recorder on the HIP embedder's own context (identical conditioning, as tests/fullsize_util.py does):
    fp64 is the truth, the oracle's fp32 run the yardstick.  `scene`: compare that scene only, on its selected points."""
    N = e1.shape[1]
    emb = md["input_embedder"](e0.to(DEV)[:, :, :cfg["input_dim"]])
    ex_dev = None if extra is None else extra.to(DEV)[:, None, :].expand(-1, N, -1)
    ws, lp = md["flow"].attention_weights(e1.to(DEV), context=emb, extra_context=ex_dev, layers=layers, points=points, eps=[e.to(DEV) for e in eps],
                                          return_log_prob=True)
    lp_ref = md["flow"].log_prob(e1.to(DEV), context=emb, extra_context=ex_dev, eps=[e.to(DEV) for e in eps])
    assert torch.equal(lp, lp_ref)
    sl = slice(None) if scene is None else slice(scene, scene + 1)
    rows = slice(None) if points is None else torch.as_tensor(points).long()
    if points is not None and torch.as_tensor(points).dim() == 2:
        assert scene is not None
        rows = torch.as_tensor(points).long()[scene]
    x = e1[sl][:, rows]
    out = {}
    for dtype in (torch.float64, torch.float32):
        sd_f, _ = state_dicts(md, dtype)
        ex = None if extra is None else extra[sl].to(dtype)[:, None, :].expand(-1, x.shape[1], -1)
        with torch.no_grad(), U.recording_oracle() as rec:
            O.flow_log_prob(cfg, sd_f, x.to(dtype), emb[sl].cpu().to(dtype), ex, [e[sl][:, rows].to(dtype) for e in eps])
        out[dtype] = dict(rec)
    prefixes = list(out[torch.float64])
    worst = 0.0
    for l, w in zip(layers, ws):
        p = next(p for p in prefixes if U.layer_of(cfg, p) == l)
        err, bound = _ratio(f"{label} layer {l}", w[sl], out[torch.float64][p], out[torch.float32][p])
        worst = max(worst, err / bound)
    return worst, ws


def test_other_head_dims_against_the_oracle():
    """Head dim 32 with an fp32 K panel (e2e_tiny_affine: 5 attentions x 64 columns are no multiple of 128, so prepare keeps fp32 K) and head
    dim 128 (inner dim 96, padded; always the fp32 panel): no reference fixture holds their weights, so the fp64 oracle recorder is the
    truth and its fp32 run the yardstick."""
    fx = Fixture("e2e_tiny_affine")
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    sd_flow, sd_emb = fx.state_dicts()
    for k in sd_flow:
        if k.endswith(".attention.to_q.weight"):
            sd_flow[k] = sd_flow[k] * 64.0                              # peaked rows
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    with _kernels() as kn:
        worst, _ = _against_oracle("e2e_tiny_affine (head dim 32, fp32 K)", cfg, md, fx.t("extract_0"), fx.t("extract_1"), fx.t("extra"), fx.eps(),
                                   ["aug", 0, 1, 2, 3])
    assert worst <= 1.0 and kn.ran("attn_weights_kernel<32, 0>") and not kn.ran("attn_weights_kernel<32, 1>"), kn.names
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=2, sample_size=150, cross_heads=1, cross_dim_head=96)
    torch.manual_seed(5)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    with torch.no_grad():
        for n, p in md["flow"].named_parameters():
            if n.endswith(".attention.to_q.weight"):
                p.mul_(32.0)
    e0, e1, extra, eps = synth_pairs(2, 333, 150, 6, cfg["latent_dim"] - cfg["input_dim"])
    with _kernels() as kn:
        worst, ws = _against_oracle("inner dim 96 (head dim 128)", cfg, md, e0, e1, extra, [eps], ["aug", 0, 1])
    assert worst <= 1.0 and tuple(ws[0].shape) == (2, 150, 333) and kn.ran("attn_weights_kernel<128, 0>"), kn.names


def test_range_fallback_pass_rewrites_the_weights():
    """The recipe of test_gpu_flow.test_out_of_fp16_range_activations_repeat_on_the_bf16_limb_path: hidden activations of ~1e6 in one coupling
    net raise the fp16 range flag, the pass repeats on the bf16 limbs (no guard scope: three-launch q, fp32 K) and rewrites the weight
    buffers.  Against the fp64 oracle recorder, gated at 4 x the oracle's own fp32-vs-fp64 error; the log-prob equals inner_loop's."""
    lib = engine.lib()
    fx = Fixture("e2e_tiny_spline_relu")
    cfg = dict(fx.cfg)
    sd_flow, sd_emb = fx.state_dicts()
    pre = "transforms.4.transform.nn."
    for k in sd_flow:
        if k.startswith(pre + "in_layer.") or (k.startswith(pre + "layers.") and k.endswith(".bias")):
            sd_flow[k] = sd_flow[k] * 1.0e6
        elif k == pre + "out_layer.weight":
            sd_flow[k] = sd_flow[k] / 1.0e6
        elif k.endswith(".attention.to_q.weight"):
            sd_flow[k] = sd_flow[k] * 64.0
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    before = lib.fc_debug_fp16_fallbacks()
    worst, ws = _against_oracle("range fallback (e2e_tiny_spline_relu, alpha 1e6)", cfg, md, fx.t("extract_0"), fx.t("extract_1"), fx.t("extra"),
                                fx.eps(), ["aug", 0, 1, 2])
    assert lib.fc_debug_fp16_fallbacks() >= before + 2, "the passes were expected to repeat on the bf16 limbs"
    assert worst <= 1.0
    batch, eps = _fixture_inputs(fx)
    with engine.deferred_range_check() as drc:                      # the repeat at resolve() rewrites buffers the call has long returned
        dws, dlp = fa.attention_weights(batch, md, cfg, layers=["aug", 0, 1, 2], eps=eps, return_log_prob=True)
    assert drc.repeated >= 1
    torch.cuda.synchronize()
    assert torch.equal(dlp, fa.inner_loop(batch, md, cfg, eps=eps)[1])
    for a, b in zip(dws, ws):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 5. size
def test_native_shape_three_maps_two_points_per_scene():
    """The reference's native shape (20 scenes x 1024 targets, 1250 context points, 115 layers, conditioned weights) with the reference
    script's request: layers ("aug", 50, 110), 2 points per scene.  Scene 0 against the fp64 oracle recorder (the two selected points run
    through all 115 layers there: points do not interact), the oracle's fp32 run as the yardstick."""
    B, N, M = 20, 1024, 1250
    cfg, md = build_conditioned("c4_dgcnn_attn_extra_affine", N, DEV)
    e0, e1, extra, eps = synth_pairs(B, M, N, 21, cfg["latent_dim"] - cfg["input_dim"])
    idx = torch.randint(0, N, (B, 2), generator=torch.Generator().manual_seed(3))
    worst, ws = _against_oracle("native shape", cfg, md, e0, e1, extra, [eps], ["aug", 50, 110], points=idx, scene=0)
    for w in ws:
        assert tuple(w.shape) == (B, 2, M)                          # 1250 columns: not a tile multiple
        assert torch.isfinite(w).all() and (w >= 0).all()
        assert (w.double().sum(-1) - 1.0).abs().max().item() <= M * 2.0 ** -23
    assert worst <= 1.0
    batch = (e0.to(DEV), e1.to(DEV), extra.to(DEV))
    via_fa = fa.attention_weights(batch, md, cfg, layers=("aug", 50, 110), points=idx, eps=[eps.to(DEV)])
    for a, b in zip(via_fa, ws):
        assert torch.equal(a, b)


def test_full_map_at_c2_size():
    """One full map at C2's 16 x 4096 targets / 4096 context points (1 GiB) for one layer: the exact properties on it."""
    B, N = 16, 4096
    cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=2, sample_size=N)
    torch.manual_seed(11)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    e0, e1, _, eps = synth_pairs(B, N, N, 12)
    batch = (e0.to(DEV), e1.to(DEV), None)
    eps = [eps.to(DEV)]
    _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    (w,), lp_w = fa.attention_weights(batch, md, cfg, layers=(1,), eps=eps, return_log_prob=True)
    assert tuple(w.shape) == (B, N, N) and torch.equal(lp_w, lp)
    for b in range(B):
        assert torch.isfinite(w[b]).all() and (w[b] >= 0).all()
        assert (w[b].double().sum(-1) - 1.0).abs().max().item() <= N * 2.0 ** -23
    idx = torch.randint(0, N, (B, 3), generator=torch.Generator().manual_seed(4))
    (sel,) = fa.attention_weights(batch, md, cfg, layers=(1,), points=idx, eps=eps)
    assert torch.equal(sel, torch.stack([w[b, idx[b].to(DEV)] for b in range(B)]))
    keep = w[:, :64].clone()
    del w
    (w2,) = fa.attention_weights(batch, md, cfg, layers=(1,), eps=eps)
    assert torch.equal(w2[:, :64], keep)


# ------------------------------------------------------------------ 6. errors, before any launch
def test_errors_name_their_cause_and_leave_the_stream_usable():
    fx = Fixture("e2e_c1_global_L2")
    cfg, md = _build(fx)
    batch, eps = _fixture_inputs(fx)
    with pytest.raises(RuntimeError, match="no attention.*global-context"):
        fa.attention_weights(batch, md, cfg, layers=(0,), eps=eps)
    with pytest.raises(RuntimeError, match="no attention.*global-context"):
        fa.attention_weights(batch, md, cfg, layers=("aug", 1), eps=eps)
    (w,) = fa.attention_weights(batch, md, cfg, layers=("aug",), eps=eps)        # the augmenter of a global-context flow still attends
    assert tuple(w.shape) == (fx.meta["B"], fx.meta["N"], fx.meta["N"]) and (w.double().sum(-1) - 1).abs().max().item() <= fx.meta["N"] * 2.0 ** -23
    with pytest.raises(RuntimeError, match="out of range"):
        fa.attention_weights(batch, md, cfg, layers=(2,), eps=eps)
    h = md["flow"]._engine()
    emb = md["input_embedder"](batch[0])[:, None, :].expand(-1, fx.meta["N"], -1)
    with pytest.raises(RuntimeError, match="layer id 7 is out of range"):         # the C entry checks too
        h.attention_weights(batch[1], emb, None, eps, [7])
    with pytest.raises(RuntimeError, match="layer id -2 is out of range"):
        h.attention_weights(batch[1], emb, None, eps, [-2])
    with pytest.raises(RuntimeError, match=r"index 64 is not in \[0, 64\)"):
        fa.attention_weights(batch, md, cfg, layers=("aug",), points=[0, 64], eps=eps)
    with pytest.raises(RuntimeError, match="integer index tensor"):
        fa.attention_weights(batch, md, cfg, layers=("aug",), points=torch.tensor([0.0, 1.0]), eps=eps)
    md["flow"].train()
    with pytest.raises(RuntimeError, match="eval-mode only"):
        fa.attention_weights(batch, md, cfg, layers=("aug",), eps=eps)
    md["flow"].eval()
    _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    assert np.abs(lp.cpu().double().numpy() - fx.a["log_prob_f64"]).max() < 2e-3

    fx = Fixture("e2e_tiny_identity_aug")
    cfg, md = _build(fx)
    batch, eps = _fixture_inputs(fx)
    with pytest.raises(RuntimeError, match="IdentityTransform"):
        fa.attention_weights(batch, md, cfg, layers=("aug",), eps=eps)
    ws = fa.attention_weights(batch, md, cfg, layers=(0, 2), points=[1], eps=eps)
    assert len(ws) == 2 and tuple(ws[0].shape) == (fx.meta["B"], 1, fx.meta["M"])
    _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    assert np.abs(lp.cpu().double().numpy() - fx.a["log_prob_f64"]).max() < 2e-3
    with pytest.raises(RuntimeError, match="D must be 32, 64 or 128"):
        engine.op_attention_weights(torch.zeros(1, 4, 48, device=DEV), torch.zeros(1, 4, 48, device=DEV), 1.0)
