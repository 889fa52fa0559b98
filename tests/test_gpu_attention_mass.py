"""fa.attention_mass / fc_flow_attention_mass_f32 / fc_op_attention_mass_f32 (csrc/attention_mass.hip) on the GPU: the weighted column sums
   mass[b, j] = sum_p g[b, p] * softmax_j(q[b, p, :] . k[b, j, :])
of the cross-attention maps that fa.attention_weights exports row by row, reduced on the chip.

Gate wherever a comparison with fp64 is made (gate()):  max |m - m64| <= 4 x E,  E = max(max |m32 - m64|, (N + 4) * 2^-24 * max |m64|),
with m32 the same quantity from an fp32 evaluation that is NOT the code under test (torch on the CPU, the reference's fp32 run in the
fixture, the oracle in fp32); the floor is the order-independent bound on an fp32 sum of N terms.  Every test prints the measured ratio
max |m - m64| / E before it asserts."""
import contextlib
import io

import numpy as np
import pytest
import torch

import attn_weights_util as U
import flowcompare_amd as fa
import knob_util
import scene_stage_util as SU
from conftest import Fixture
from flowcompare_amd import change, engine, staging
from fullsize_util import state_dicts, synth_pairs
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FC_ERR_WORKSPACE = 4


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


def gate(err_f32, mmax, N):
    return 4.0 * max(float(err_f32), (N + 4) * 2.0 ** -24 * float(mmax))


def _ratio(label, m, m64, m32, N):
    """prints max |m - m64| / E and returns (error, 4 E)"""
    m, m64, m32 = (torch.as_tensor(t).double().cpu() for t in (m, m64, m32))
    err, e32, mmax = (m - m64).abs().max().item(), (m32 - m64).abs().max().item(), m64.abs().max().item()
    bound = gate(e32, mmax, N)
    print(f"{label}: max |m - fp64| {err:.2e}   fp32 yardstick {e32:.2e}   max |m| {mmax:.3e}   ratio to E {4.0 * err / bound:.2f}  (gate 4)")
    return err, bound


# ------------------------------------------------------------------ 1 - 3. the operator: fp64, the exported map, conservation
SHAPES = [(1, 1, 1, 32), (2, 33, 1, 64), (1, 31, 65, 32), (3, 100, 130, 64), (2, 129, 63, 64), (2, 257, 1000, 64), (2, 40, 70, 128),
          (1, 130, 200, 256), (1, 4096, 4096, 64)]
WEIGHTS = ["ones", "uniform", "normal", "mask"]
_case_cache = {}


def _weights(kind, B, N):
    """None, uniform in [0, 1), signed normal, or a 0/1 mask whose rows 32..63 (a whole wave's block) and 128..255 (a whole
    workgroup's) are zero"""
    if kind == "ones":
        return None
    gen = torch.Generator().manual_seed(40 + WEIGHTS.index(kind))
    if kind == "uniform":
        return torch.rand(B, N, generator=gen)
    if kind == "normal":
        return torch.randn(B, N, generator=gen)
    g = (torch.rand(B, N, generator=gen) < 0.5).float()
    g[:, 32:64] = 0.0
    g[:, 128:256] = 0.0
    return g


def _case(B, N, M, D):
    """inputs and references of one shape, computed once and shared by the tests: q, k, the softmax in fp64 and in eager fp32 on the
    CPU, and this build's own full map"""
    key = (B, N, M, D)
    if key not in _case_cache:
        q, k = _rand(B, N, D, seed=1, scale=2.0), _rand(B, M, D, seed=2, scale=2.0)
        sm = D ** -0.5
        w64 = torch.softmax((q.double() @ k.double().transpose(1, 2)) * sm, -1)
        w32 = torch.softmax((q @ k.transpose(1, 2)) * sm, -1)
        W = engine.op_attention_weights(q.to(DEV), k.to(DEV), sm).cpu()
        _case_cache[key] = (q.to(DEV), k.to(DEV), sm, w64, w32, W)
    return _case_cache[key]


def _g64(g, B, N):
    return torch.ones(B, N, dtype=torch.float64) if g is None else g.double()


@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("B,N,M,D", SHAPES)
def test_operator_matches_fp64(B, N, M, D, kind):
    q, k, sm, w64, w32, _ = _case(B, N, M, D)
    g = _weights(kind, B, N)
    m = engine.op_attention_mass(q, k, sm, weights=None if g is None else g.to(DEV)).cpu()
    assert tuple(m.shape) == (B, M) and m.dtype == torch.float32 and torch.isfinite(m).all()
    g64 = _g64(g, B, N)
    m64 = (g64[:, :, None] * w64).sum(1)
    m32 = (g64.float()[:, :, None] * w32).sum(1)                       # the same formula in eager fp32 on the CPU
    err, bound = _ratio(f"B {B} N {N} M {M} D {D} g {kind}", m, m64, m32, N)
    assert err <= bound
    if M == 1:                                                          # every row is the single weight 1: the mass is sum_p g
        tot = g64.sum(1, keepdim=True)
        assert ((m.double() - tot).abs() <= (N + 4) * 2.0 ** -24 * g64.abs().sum(1, keepdim=True)).all()


@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("B,N,M,D", SHAPES)
def test_operator_is_the_column_sum_of_the_exported_map(B, N, M, D, kind):
    """The probabilities are the bits op_attention_weights stores; only the products with g and the summation round:
    |m - sum64(g W)| <= (N + 4) 2^-24 sum_p |g_p| W_pj, element by element."""
    q, k, sm, _, _, W = _case(B, N, M, D)
    g = _weights(kind, B, N)
    m = engine.op_attention_mass(q, k, sm, weights=None if g is None else g.to(DEV)).cpu().double()
    g64 = _g64(g, B, N)
    s64 = (g64[:, :, None] * W.double()).sum(1)
    bound = (N + 4) * 2.0 ** -24 * (g64.abs()[:, :, None] * W.double()).sum(1)
    excess = ((m - s64).abs() - bound).max().item()
    worst = ((m - s64).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"B {B} N {N} M {M} D {D} g {kind}: max |m - sum64(g W)| / bound {worst:.3f}")
    assert excess <= 0.0


@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("B,N,M,D", SHAPES)
def test_mass_is_conserved(B, N, M, D, kind):
    """sum_j m[b, j] = sum_p g[b, p] within the row-sum bound of the weight tests (M 2^-23 per row) plus the summation's."""
    q, k, sm, _, _, _ = _case(B, N, M, D)
    g = _weights(kind, B, N)
    m = engine.op_attention_mass(q, k, sm, weights=None if g is None else g.to(DEV)).cpu().double()
    g64 = _g64(g, B, N)
    gap = (m.sum(1) - g64.sum(1)).abs()
    bound = (M * 2.0 ** -23 + (N + 4) * 2.0 ** -24) * g64.abs().sum(1)
    print(f"B {B} N {N} M {M} D {D} g {kind}: max |sum_j m - sum_p g| / bound {(gap / bound.clamp_min(1e-300)).max().item():.3f}")
    assert (gap <= bound).all()


# ------------------------------------------------------------------ 4. determinism and independence
def test_two_calls_give_the_same_bytes_and_zero_weight_means_zero_contribution():
    B, N, M, D = 2, 300, 333, 64
    q, k = _rand(B, N, D, seed=11, scale=2.0).to(DEV), _rand(B, M, D, seed=12, scale=2.0).to(DEV)
    g = torch.rand(B, N, generator=torch.Generator().manual_seed(13)).to(DEV)
    a, b = engine.op_attention_mass(q, k, 0.125, weights=g), engine.op_attention_mass(q, k, 0.125, weights=g)
    assert torch.equal(a, b)
    assert torch.equal(engine.op_attention_mass(q, k, 0.125), engine.op_attention_mass(q, k, 0.125, weights=torch.ones(N, device=DEV)))
    assert torch.equal(engine.op_attention_mass(q, k, 0.125, weights=g > 0.5), engine.op_attention_mass(q, k, 0.125, weights=(g > 0.5).float()))
    off = torch.zeros(B, N, dtype=torch.bool)
    off[:, [0, 5, 31, 32, 127, 128, 255, 299]] = True
    off[1, 64:96] = True
    g0 = torch.where(off.to(DEV), torch.zeros_like(g), g)
    bad = q.clone()
    junk = torch.tensor([1e30, -1e30, float("nan"), float("inf"), 3.0e4, -7.0], device=DEV).repeat(11)[:D]
    bad[off.to(DEV)] = junk
    assert torch.equal(engine.op_attention_mass(q, k, 0.125, weights=g0), engine.op_attention_mass(bad, k, 0.125, weights=g0))
    assert not torch.equal(engine.op_attention_mass(q, k, 0.125, weights=g0), a)


@pytest.mark.parametrize("per_tile", [0.4, 1.5, 7.5])
def test_operator_score_ramps(per_tile):
    """Scores that rise along the key axis (test_gpu_attention_weights.test_operator_score_ramps): the running maximum of pass 1 moves in
    every tile, and the last tiles hold all the mass."""
    B, N, M, D = 2, 200, 1024, 64
    q, k = _rand(B, N, D, seed=61), _rand(B, M, D, seed=62)
    q[..., 0] = 4.0
    k[..., 0] = torch.arange(M).float()[None, :] * (per_tile / 64.0 / (0.125 * 4.0))
    g = torch.rand(B, N, generator=torch.Generator().manual_seed(63))
    w64 = torch.softmax((q.double() @ k.double().transpose(1, 2)) * 0.125, -1)
    w32 = torch.softmax((q @ k.transpose(1, 2)) * 0.125, -1)
    m = engine.op_attention_mass(q.to(DEV), k.to(DEV), 0.125, weights=g.to(DEV))
    err, bound = _ratio(f"ramp {per_tile} nats per tile", m, (g.double()[:, :, None] * w64).sum(1), (g[:, :, None] * w32).sum(1), N)
    assert err <= bound


# ------------------------------------------------------------------ 5. the engine against the reference's weights
def _build(fx):
    cfg = dict(fx.cfg)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    sd_flow, sd_emb = U.state_dicts(fx)
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    return cfg, md


def _fixture_inputs(fx):
    batch = tuple(None if t is None else t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
    return batch, [e.to(DEV) for e in fx.eps()]


def _check_masses(label, ms, w64s, w32s, g):
    """masses of a list of attentions against the column sums of their fp64 maps; returns the worst error / (4 E)"""
    worst = 0.0
    for i, m in enumerate(ms):
        w64, w32 = torch.as_tensor(w64s[i]).double(), torch.as_tensor(w32s[i]).float()
        B, N, M = w64.shape
        g64 = _g64(g, B, N)
        assert tuple(m.shape) == (B, M) and m.dtype == torch.float32 and torch.isfinite(m).all()
        err, bound = _ratio(f"{label} attention {i}", m, (g64[:, :, None] * w64).sum(1), (g64.float()[:, :, None] * w32).sum(1), N)
        worst = max(worst, err / bound)
    return worst


@pytest.mark.parametrize("case", list(U.CASES))
def test_engine_matches_reference_weights(case):
    """All attentions of each fixture against the column sums of the reference's fp64 `attn_weights`, the reference's own fp32 run as the
    yardstick.  On attnw_sharp_L3 the masses span 0.002 .. 17, so a flat answer N / M fails by orders of magnitude; on the near-uniform
    fixtures it is >= 2.7e-3 off against a gate of ~1e-5."""
    fx, ref = U.load_case(case)
    cfg, md = _build(fx)
    batch, eps = _fixture_inputs(fx)
    B, N = fx.meta["B"], fx.meta["N"]
    layers = [U.layer_of(cfg, p) for p in ref.prefixes]
    assert md["flow"].attention_layers() == layers
    _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    with _kernels() as kn:
        ms, lp_m = fa.attention_mass(batch, md, cfg, layers=layers, eps=eps, return_log_prob=True)
    assert kn.ran("attn_mass_kernel<32, 1>" if case == "e2e_tiny_cif" else "attn_mass_kernel<64, 1>"), kn.names
    assert kn.ran("attn_mass_reduce_kernel") and not kn.ran("attn_weights_kernel"), kn.names
    assert torch.equal(lp_m, lp), "the probe disturbed the pass"
    assert _check_masses(f"{case} g ones", ms, ref.w64, ref.w32, None) <= 1.0
    g = torch.rand(B, N, generator=torch.Generator().manual_seed(77))
    mg = fa.attention_mass(batch, md, cfg, layers=layers, weights=g.to(DEV), eps=eps)
    assert _check_masses(f"{case} g random", mg, ref.w64, ref.w32, g) <= 1.0
    every = fa.attention_mass(batch, md, cfg, layers="all", eps=eps)
    assert len(every) == len(ms)
    for i, l in enumerate(layers):                                      # "all" = the per-layer requests, alone and together, bit for bit
        assert torch.equal(every[i], ms[i])
        assert torch.equal(fa.attention_mass(batch, md, cfg, layers=(l,), eps=eps)[0], ms[i])
    for a, b in zip(fa.attention_mass(batch, md, cfg, layers=layers[::-1], weights=g.to(DEV), eps=eps), mg[::-1]):
        assert torch.equal(a, b)
    flat = float(N) / ref.w64[0].shape[2]
    off_flat = max((m.double().cpu() - flat).abs().max().item() for m in ms)
    print(f"{case}: a flat answer N / M = {flat:.3f} would be {off_flat:.2e} off")
    assert off_flat > 10 * gate(0.0, max(float(np.abs(w.sum(1)).max()) for w in ref.w64), N)
    # under the deferred range check the call only enqueues its pass; same bits once resolved
    with engine.deferred_range_check() as drc:
        dm, dlp = fa.attention_mass(batch, md, cfg, layers=layers, weights=g.to(DEV), eps=eps, return_log_prob=True)
    assert drc.repeated == 0 and torch.equal(dlp, lp)
    for a, b in zip(dm, mg):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 6. every operand form
# The six knob paths of test_gpu_attention_weights.test_every_operand_form_on_the_sharp_fixture, restated:
# (label, knobs, K form of the kernel, the kernels that mark the q forms of the run)
PATHS = [("row-resident chain q (augmenter: fold finished on load), limb-image K (default)", {}, 1, {"premlp_rows_kernel"}),
         ("LayerNorm -> q fold finished on load, limb-image K", {8: 0}, 1, set()),
         ("LayerNorm -> q fold + launch_lnq_finalize, fp32 K", {8: 0, 5: 0}, 0, {"lnq_finalize_kernel"}),
         ("three-launch fallback q, limb-image K", {8: 0, 10: 0}, 1, {"layernorm_kernel"}),
         ("row-resident chain q (augmenter: launch_lnq_finalize), fp32 K", {5: 0}, 0, {"premlp_rows_kernel", "lnq_finalize_kernel"}),
         ("no guard scope (bf16-limb GEMMs): three-launch q, fp32 K", {0: 3}, 0, {"layernorm_kernel"})]


@pytest.mark.parametrize("label,knobs,kform,qmarks", PATHS, ids=["default", "fold_on_load", "fold_finalize-fp32_K", "three_launch", "chain-fp32_K", "no_guard_scope"])
def test_every_operand_form_on_the_sharp_fixture(label, knobs, kform, qmarks):
    fx, ref = U.load_case(U.SHARP)
    cfg, md = _build(fx)
    batch, eps = _fixture_inputs(fx)
    layers = [U.layer_of(cfg, p) for p in ref.prefixes]
    g = torch.rand(fx.meta["B"], fx.meta["N"], generator=torch.Generator().manual_seed(78))
    with _kernels() as kn, knob_util.knobs(knobs):
        ms = fa.attention_mass(batch, md, cfg, layers=layers, weights=g.to(DEV), eps=eps)
    assert _check_masses(f"{U.SHARP} [{label}]", ms, ref.w64, ref.w32, g) <= 1.0
    assert kn.ran(f"attn_mass_kernel<64, {kform}>") and not kn.ran(f"attn_mass_kernel<64, {1 - kform}>"), kn.names
    for mark in ("premlp_rows_kernel", "lnq_finalize_kernel", "layernorm_kernel"):
        assert kn.ran(mark) == (mark in qmarks), (mark, kn.names)


def _against_oracle(label, cfg, md, e0, e1, extra, eps, layers, g):
    """HIP masses against the column sums of the oracle recorder's maps on the HIP embedder's own context (identical conditioning):
    fp64 is the truth, the oracle's fp32 run the yardstick.  Returns (worst error / (4 E), the masses)."""
    N = e1.shape[1]
    emb = md["input_embedder"](e0.to(DEV)[:, :, :cfg["input_dim"]])
    ex_dev = None if extra is None else extra.to(DEV)[:, None, :].expand(-1, N, -1)
    eps_dev = [e.to(DEV) for e in eps]
    ms, lp = md["flow"].attention_mass(e1.to(DEV), context=emb, extra_context=ex_dev, layers=layers, weights=None if g is None else g.to(DEV),
                                       eps=eps_dev, return_log_prob=True)
    assert torch.equal(lp, md["flow"].log_prob(e1.to(DEV), context=emb, extra_context=ex_dev, eps=eps_dev))
    out = {}
    for dtype in (torch.float64, torch.float32):
        sd_f, _ = state_dicts(md, dtype)
        ex = None if extra is None else extra.to(dtype)[:, None, :].expand(-1, N, -1)
        with torch.no_grad(), U.recording_oracle() as rec:
            O.flow_log_prob(cfg, sd_f, e1.to(dtype), emb.cpu().to(dtype), ex, [e.to(dtype) for e in eps])
        out[dtype] = dict(rec)
    prefix = {U.layer_of(cfg, p): p for p in out[torch.float64]}
    worst = _check_masses(label, ms, [out[torch.float64][prefix[l]] for l in layers], [out[torch.float32][prefix[l]] for l in layers], g)
    return worst, ms


@pytest.mark.parametrize("inner,dh", [(96, 128), (256, 256)])
def test_other_head_dims_against_the_oracle(inner, dh):
    """Head dims 128 (inner dim 96, padded) and 256: always the fp32 K panel; no reference fixture holds their weights, so the fp64
    oracle recorder is the truth (as test_gpu_attention_weights.test_other_head_dims_against_the_oracle does for the rows)."""
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=2, sample_size=150, cross_heads=1, cross_dim_head=inner)
    torch.manual_seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    with torch.no_grad():
        for n, p in md["flow"].named_parameters():
            if n.endswith(".attention.to_q.weight"):
                p.mul_(32.0)
    e0, e1, extra, eps = synth_pairs(2, 333, 150, 6, cfg["latent_dim"] - cfg["input_dim"])
    g = torch.rand(2, 150, generator=torch.Generator().manual_seed(79))
    with _kernels() as kn:
        worst, ms = _against_oracle(f"inner dim {inner} (head dim {dh})", cfg, md, e0, e1, extra, [eps], ["aug", 0, 1], g)
    assert worst <= 1.0 and tuple(ms[0].shape) == (2, 333) and kn.ran(f"attn_mass_kernel<{dh}, 0>"), kn.names


def test_range_fallback_pass_rewrites_the_masses():
    """The recipe of test_gpu_attention_weights.test_range_fallback_pass_rewrites_the_weights: hidden activations of ~1e6 in one coupling
    net raise the fp16 range flag, the pass repeats on the bf16 limbs (no guard scope: three-launch q, fp32 K) and rewrites slabs and
    outputs.  Finite, against the fp64 oracle recorder, and the same bytes when the repeat happens at resolve()."""
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
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    g = torch.rand(fx.meta["B"], fx.meta["N"], generator=torch.Generator().manual_seed(80))
    before = lib.fc_debug_fp16_fallbacks()
    worst, ms = _against_oracle("range fallback (e2e_tiny_spline_relu, alpha 1e6)", cfg, md, fx.t("extract_0"), fx.t("extract_1"), fx.t("extra"),
                                fx.eps(), ["aug", 0, 1, 2], g)
    assert lib.fc_debug_fp16_fallbacks() >= before + 2, "the passes were expected to repeat on the bf16 limbs"
    assert worst <= 1.0 and all(torch.isfinite(m).all() for m in ms)
    batch, eps = _fixture_inputs(fx)
    with engine.deferred_range_check() as drc:                      # the repeat at resolve() rewrites buffers the call has long returned
        dms, dlp = fa.attention_mass(batch, md, cfg, layers=["aug", 0, 1, 2], weights=g.to(DEV), eps=eps, return_log_prob=True)
    assert drc.repeated >= 1
    torch.cuda.synchronize()
    assert torch.equal(dlp, fa.inner_loop(batch, md, cfg, eps=eps)[1])
    for a, b in zip(dms, ms):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 7. a plain forward is untouched
def test_a_plain_forward_launches_no_mass_kernel_and_keeps_its_workspace():
    import ctypes
    fx, ref = U.load_case(U.SHARP)
    cfg, md = _build(fx)
    batch, eps = _fixture_inputs(fx)
    B, N, M = fx.meta["B"], fx.meta["N"], fx.meta["M"]
    lib, h = engine.lib(), md["flow"]._engine()

    def ws_bytes(entry):
        n = ctypes.c_size_t()
        entry(h._h, B, N, M, ctypes.byref(n))
        return n.value
    fwd = ws_bytes(lib.fc_flow_workspace_bytes)
    with _kernels() as kn:
        _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    plain = list(kn.names)
    assert plain and not kn.ran("attn_mass") and not kn.ran("attn_weights_kernel"), kn.names
    with _kernels() as kn:
        fa.attention_mass(batch, md, cfg, layers=("aug", 1), eps=eps)
    assert kn.ran("attn_mass_kernel<64, 1>") and kn.ran("attn_mass_reduce_kernel")
    assert sorted(set(kn.names) - set(plain)) == sorted(n for n in set(kn.names) if "attn_mass" in n), "only the two mass kernels are added"
    assert ws_bytes(lib.fc_flow_workspace_bytes) == fwd
    slab = lib.fc_op_attention_mass_scratch_bytes(B, N, M)
    assert fwd + slab <= ws_bytes(lib.fc_flow_attention_mass_workspace_bytes) <= fwd + slab + 256
    with _kernels() as kn:
        assert torch.equal(fa.inner_loop(batch, md, cfg, eps=eps)[1], lp)
    assert sorted(kn.names) == sorted(plain)


# ------------------------------------------------------------------ 8. errors, before any launch
def test_errors_name_their_cause_and_leave_the_stream_usable():
    fx = Fixture("e2e_c1_global_L2")
    cfg, md = _build(fx)
    batch, eps = _fixture_inputs(fx)
    B, N = fx.meta["B"], fx.meta["N"]
    with pytest.raises(RuntimeError, match="no attention.*global-context"):
        fa.attention_mass(batch, md, cfg, layers=(0,), eps=eps)
    with pytest.raises(RuntimeError, match="no attention.*global-context"):
        fa.attention_mass(batch, md, cfg, layers=("aug", 1), eps=eps)
    (m,) = fa.attention_mass(batch, md, cfg, layers=("aug",), eps=eps)          # the augmenter of a global-context flow still attends
    assert tuple(m.shape) == (B, N) and (m.double().sum(1) - N).abs().max().item() <= (N * 2.0 ** -23 + (N + 4) * 2.0 ** -24) * N
    assert md["flow"].attention_layers() == ["aug"] and torch.equal(fa.attention_mass(batch, md, cfg, layers="all", eps=eps)[0], m)
    with pytest.raises(RuntimeError, match="out of range"):
        fa.attention_mass(batch, md, cfg, layers=(2,), eps=eps)
    with pytest.raises(RuntimeError, match="unknown layer 'first'"):
        fa.attention_mass(batch, md, cfg, layers=("first",), eps=eps)
    h = md["flow"]._engine()
    emb = md["input_embedder"](batch[0])[:, None, :].expand(-1, N, -1)
    with pytest.raises(RuntimeError, match="fc_flow_attention_mass_f32: layer id 7 is out of range"):         # the C entry checks too
        h.attention_mass(batch[1], emb, None, eps, [7])
    with pytest.raises(RuntimeError, match="layer id -2 is out of range"):
        h.attention_mass(batch[1], emb, None, eps, [-2])
    for bad, msg in ((torch.ones(N + 1, device=DEV), "shape"), (torch.ones(B + 1, N, device=DEV), "shape"), (torch.ones(B, N, 1, device=DEV), "shape"),
                     (torch.ones(B, N), "no CPU path"), (torch.ones(B, N, device=DEV, dtype=torch.int64), "float or bool"),
                     (torch.full((B, N), float("nan"), device=DEV), "finite"), (torch.full((N,), float("inf"), device=DEV), "finite"),
                     ([1.0] * N, "tensor")):
        with pytest.raises(RuntimeError, match=msg):
            fa.attention_mass(batch, md, cfg, layers=("aug",), weights=bad, eps=eps)
    md["flow"].train()
    with pytest.raises(RuntimeError, match="eval-mode only"):
        fa.attention_mass(batch, md, cfg, layers=("aug",), eps=eps)
    md["flow"].eval()
    # scratch / workspace too small: FC_ERR_WORKSPACE, named
    q, k, out = torch.zeros(1, 200, 64, device=DEV), torch.zeros(1, 70, 64, device=DEV), torch.zeros(1, 70, device=DEV)
    need = engine.lib().fc_op_attention_mass_scratch_bytes(1, 200, 70)
    scratch = torch.zeros(need, dtype=torch.uint8, device=DEV)
    with pytest.raises(engine.FcError, match="scratch too small") as err:
        engine.lib().fc_op_attention_mass_f32(q.data_ptr(), k.data_ptr(), None, out.data_ptr(), 1, 200, 70, 64, 1.0, scratch.data_ptr(), need - 1, None)
    assert err.value.code == FC_ERR_WORKSPACE
    with pytest.raises(engine.FcError, match="D must be 32, 64, 128 or 256"):
        engine.op_attention_mass(torch.zeros(1, 4, 48, device=DEV), torch.zeros(1, 4, 48, device=DEV), 1.0)
    import ctypes
    n = ctypes.c_size_t()
    engine.lib().fc_flow_workspace_bytes(h._h, B, N, N, ctypes.byref(n))
    ws = torch.zeros(n.value, dtype=torch.uint8, device=DEV)                # the forward's workspace alone: no room for the slabs
    x = batch[1].contiguous()
    ctx = emb.contiguous()
    eps_arr = (ctypes.c_void_p * 1)(eps[0].contiguous().data_ptr())
    lay, outs = (ctypes.c_int32 * 1)(-1), (ctypes.c_void_p * 1)(m.data_ptr())
    with pytest.raises(engine.FcError, match="workspace too small") as err:
        engine.lib().fc_flow_attention_mass_f32(h._h, x.data_ptr(), ctx.data_ptr(), None, eps_arr, 1, lay, 1, None, outs, None, B, N, N, ws.data_ptr(),
                                                ws.numel(), None)
    assert err.value.code == FC_ERR_WORKSPACE
    _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    assert np.abs(lp.cpu().double().numpy() - fx.a["log_prob_f64"]).max() < 2e-3
    assert torch.equal(fa.attention_mass(batch, md, cfg, layers=("aug",), eps=eps)[0], m)

    fx = Fixture("e2e_tiny_identity_aug")
    cfg, md = _build(fx)
    batch, eps = _fixture_inputs(fx)
    with pytest.raises(RuntimeError, match="IdentityTransform"):
        fa.attention_mass(batch, md, cfg, layers=("aug",), eps=eps)
    ms = fa.attention_mass(batch, md, cfg, layers=(0, 2), eps=eps)
    assert len(ms) == 2 and tuple(ms[0].shape) == (fx.meta["B"], fx.meta["M"])
    assert "aug" not in md["flow"].attention_layers()
    _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    assert np.abs(lp.cpu().double().numpy() - fx.a["log_prob_f64"]).max() < 2e-3


# ------------------------------------------------------------------ 9. the scene-level entry
@pytest.fixture(scope="module")
def scene():
    c0, c1 = SU.scene()
    return torch.from_numpy(c0).to(DEV), torch.from_numpy(c1).to(DEV), torch.from_numpy(SU.centers_np()).to(DEV)


def _scene_model(**kw):
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=2, sample_size=SU.N_SAMPLES, n_samples_context=SU.N_CONTEXT, **kw)
    cfg["final_voxel_size"], cfg["context_voxel_size"] = SU.FINAL, SU.CONTEXT
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
    return cfg, md


def _same(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(-1.0), b.nan_to_num(-1.0))


@pytest.mark.parametrize("weight", ["change", "uniform"])
def test_scene_context_attribution_equals_the_hand_written_composition(scene, weight):
    """An untrained two-layer flow with an augmenter (it draws noise) on the synthetic scene, 30 valid voxels in chunks of 7 (the last
    chunk holds 2).  Bit-equal to the composition written out below; NaN exactly on the rows of cloud 0 that no evaluated voxel sampled
    as context."""
    c0, c1, centers = scene
    cfg, md = _scene_model(latent_dim=16, cif_latent_dim=16)
    layers = ["aug", 1]
    kw = dict(ground_height=SU.GROUND, multiple=1.0, voxels_per_batch=7)
    torch.manual_seed(11)
    mass_0, change_1, st = fa.scene_context_attribution(c0, c1, md, cfg, centers, layers=layers, weight=weight, **kw)
    assert tuple(mass_0.shape) == (2, c0.shape[0]) and tuple(change_1.shape) == (c1.shape[0],) and mass_0.dtype == torch.float32

    n, m = SU.N_SAMPLES, SU.N_CONTEXT
    ok = (staging.voxel_counts(c0, centers, SU.CONTEXT) >= m) & (staging.voxel_counts(c1, centers, SU.FINAL) >= n) & \
        (staging.voxel_counts(c0, centers, SU.FINAL) >= n)
    assert int(ok.sum()) == 30
    sel = centers[ok].contiguous()
    s10 = staging.stage_scene(c0, c1, sel, SU.FINAL, SU.CONTEXT, n, m, SU.GROUND)
    s00 = staging.stage_scene(c0, c0, sel, SU.FINAL, SU.CONTEXT, n, m, SU.GROUND)
    torch.manual_seed(11)
    chunks, masses = [], []
    for a in range(0, 30, 7):
        ex = s10.extra_context[a:a + 7]
        b10 = (s10.extract_0[a:a + 7], s10.extract_1[a:a + 7], ex)
        eps = [torch.randn(s, device=DEV) for s in md["flow"].noise_shapes(b10[1].shape[0], n)]
        assert len(eps) == 1
        _, a10, _ = fa.inner_loop(b10, md, cfg, eps=eps)
        _, a00, _ = fa.inner_loop((s00.extract_0[a:a + 7], s00.extract_1[a:a + 7], ex), md, cfg, eps=eps)
        ch = change.log_prob_to_change(a10, a00, 1.0)
        chunks.append(ch)
        masses.append(torch.stack(fa.attention_mass(b10, md, cfg, layers=layers, weights=ch if weight == "change" else None, eps=eps)))
    assert masses[-1].shape == (2, 2, m)                                # the ragged last chunk
    ref_c = torch.full((c1.shape[0],), float("nan"), device=DEV)
    ref_c.scatter_reduce_(0, s10.index_1.reshape(-1), torch.cat(chunks).reshape(-1), "amax", include_self=False)
    ref_m = torch.full((2, c0.shape[0]), float("nan"), device=DEV)
    for i in range(2):
        ref_m[i].scatter_reduce_(0, s10.index_0.reshape(-1), torch.cat([mm[i] for mm in masses]).reshape(-1), "amax", include_self=False)
    assert _same(change_1, ref_c) and _same(mass_0, ref_m)
    touched = torch.zeros(c0.shape[0], dtype=torch.bool, device=DEV)
    touched[s10.index_0.reshape(-1)] = True
    assert 0 < int(touched.sum()) < c0.shape[0]
    for i in range(2):
        assert torch.equal(mass_0[i].isnan(), ~touched) and torch.equal(torch.isfinite(mass_0[i]), touched)
    assert torch.equal(st.index_0, s10.index_0) and st.voxel.tolist() == torch.nonzero(ok).flatten().tolist()
    assert float(mass_0[:, touched].min()) >= 0.0 and bool((mass_0[:, touched] > 0).any())
    if weight == "uniform":                                             # conservation per voxel survives the scatter only as an upper bound
        assert float(mass_0[:, touched].max()) <= n * (1 + 1e-5)


def test_scene_context_attribution_change_equals_scene_change(scene):
    """change_1 against fa.scene_change under the same seed, bit for bit.  scene_change lets each of its two inner_loop calls per chunk
    draw its own noise, scene_context_attribution draws one set per chunk for all three passes: the two consume the generator
    differently whenever the flow draws noise at all, so the bit-equality is a statement about a flow that draws none (latent_dim ==
    input_dim: IdentityTransform in front, no CIF) -- the only kind for which both are the same function of the seed."""
    c0, c1, centers = scene
    cfg, md = _scene_model(latent_dim=6, cif_latent_dim=6)
    assert md["flow"].noise_shapes(7, SU.N_SAMPLES) == []
    kw = dict(ground_height=SU.GROUND, multiple=1.0, voxels_per_batch=7)
    torch.manual_seed(11)
    mass_0, change_1, st = fa.scene_context_attribution(c0, c1, md, cfg, centers, layers="all", **kw)
    torch.manual_seed(11)
    ref, st_ref = fa.scene_change(c0, c1, md, cfg, centers, **kw)
    assert _same(change_1, ref) and int(torch.isfinite(ref).sum()) > 0
    assert tuple(mass_0.shape) == (2, c0.shape[0]) and torch.equal(st.index_1, st_ref.index_1) and st.voxel.tolist() == st_ref.voxel.tolist()
    with pytest.raises(RuntimeError, match="IdentityTransform"):
        fa.scene_context_attribution(c0, c1, md, cfg, centers, layers=("aug",), **kw)
    with pytest.raises(RuntimeError, match="weight must be"):
        fa.scene_context_attribution(c0, c1, md, cfg, centers, layers=(0,), weight="none", **kw)
