"""Per-scene context point counts on the GPU (include/fcflow_context_counts.h; csrc/attention.hip, attention_weights.hip, attention_mass.hip,
misc.hip zero_pad_rows_kernel, flow_engine.cpp prepare): scene b of a padded batch attends over its first count_b
context rows and gives what it gives when it is passed alone with that slice -- through the EXISTING entries, so every bit-for-bit comparison
below has the parent's code on its other side.  The fp64 bounds are those of the existing tests of the same kernels (named where used).
Which kernels ran is read from the in-library profiler."""
import contextlib
import functools
import math

import pytest
import torch

import flowcompare_amd as fa
from flowcompare_amd import engine
from knob_util import knobs
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PER_POINT_TOL = 2e-3             # the gate tests/test_gpu_attention_fold.py applies to its C2 layer stack against the fp64 oracle
SHARED = "attn16_kernel<64, 1>"  # the shared-tile kernel; the two-image kernel reports as attn16_kernel<64>

# (B, N, M, counts): limb kernels -- one full 128-query workgroup plus two rows; counts at M, at a tile edge, one tile, one key / either side of
# a tile edge, two tiles + 1, two keys.  fp32 kernels -- counts around the 64-key tile (D = 64, 128) and the 32-key tile (D = 256)
LIMB_CASES = [(4, 130, 130, (130, 128, 64, 1)), (4, 130, 130, (65, 63, 129, 2))]
FP32_CASE = (6, 40, 70, (70, 64, 33, 32, 31, 1))
ENGINE_COUNTS = (200, 137, 64, 40)


class _kernels:
    """{kernel name: launches} of the launches inside the block (the helper of tests/test_gpu_attention_fold.py)"""

    def __enter__(self):
        engine.profile_enable(True)
        engine.profile_reset()
        self.launches = {}
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                torch.cuda.synchronize()
                self.launches = {r["kernel"]: r["launches"] for r in engine.profile_report()}
        finally:
            engine.profile_enable(False)
            engine.profile_reset()
        return False

    def ran(self, substr):
        return any(substr in n for n in self.launches)


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _uniform(*shape, seed, scale=1.0):
    """the _rand of tests/test_gpu_ops.py: uniform on [-scale, scale]"""
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * scale


def _cnt(counts):
    return torch.tensor(counts, dtype=torch.int32, device=DEV)


def _attend(kind, q, k, v, sm, counts=None):
    """kind "kv": op_attention; "ctx": op_attention_ctx with k as the one tensor (v is not read)"""
    if kind == "ctx":
        return engine.op_attention_ctx(q, k, sm, counts=counts)
    return engine.op_attention(q, k, v, sm, counts=counts)


def _fp64(q, k, v, sm, counts):
    """softmax over the first count_b keys, in double"""
    out = []
    for b, c in enumerate(counts):
        w = torch.softmax((q[b].double() @ k[b, :c].double().T) * sm, -1)
        out.append(w @ v[b, :c].double())
    return torch.stack(out)


def _expected_kernel(kind, D, fp16):
    if not fp16 or D > 64:
        return f"attn_kernel<{D}>"
    return SHARED if (kind == "ctx" and D == 64) else f"attn16_kernel<{D}>"


OPERATOR_CASES = ([("ctx", 1, D, case) for D in (64, 32) for case in LIMB_CASES] + [("kv", 1, D, case) for D in (64, 32) for case in LIMB_CASES] +
                  [("kv", 0, D, FP32_CASE) for D in (64, 128, 256)] + [("ctx", 0, 64, FP32_CASE)])


# ------------------------------------------------------------------ 1. operators, bit for bit against the scene alone
@pytest.mark.parametrize("kind,fp16,D,case", OPERATOR_CASES)
def test_operator_with_counts_equals_every_scene_alone_bit_for_bit(kind, fp16, D, case):
    B, N, M, counts = case
    q, k, v = _rand(B, N, D, seed=71).to(DEV), _rand(B, M, D, seed=72, scale=2.0).to(DEV), _rand(B, M, D, seed=73).to(DEV)
    sm = D ** -0.5
    with knobs({5: fp16}):
        with _kernels() as kn:
            y = _attend(kind, q, k, v, sm, _cnt(counts))
        want = _expected_kernel(kind, D, fp16)
        assert kn.ran(want) and sum("attn" in n and "kernel<" in n for n in kn.launches) == 1, (want, kn.launches)
        for b, c in enumerate(counts):
            with _kernels() as kn1:
                alone = _attend(kind, q[b:b + 1], k[b:b + 1, :c], v[b:b + 1, :c], sm)      # the existing entry
            assert kn1.ran(want), (want, kn1.launches)
            assert torch.equal(y[b:b + 1], alone), (kind, fp16, D, b, c)


# ------------------------------------------------------------------ 2. operators against fp64
@pytest.mark.parametrize("scale", [1.0, 40.0, 0.05])
@pytest.mark.parametrize("kind,D,case", [(kind, D, case) for kind in ("ctx", "kv") for D in (64, 32) for case in LIMB_CASES])
def test_limb_kernels_with_counts_against_fp64(kind, D, case, scale):
    """2e-6 of the operand scale with q, k and v of order 1, 40 and 0.05: the bound of test_shared_tile_attention_against_fp64
    (tests/test_gpu_attention_fold.py) and test_attention_one_accumulator_form_against_fp64 (tests/test_gpu_ops.py).
    All three operands are drawn AT the scale.  The second of those tests draws v at twice the scale and still divides the error by the scale;
    its scenes have 33 keys and more, whose weighted mean is well below a single |v|.  A scene of two keys returns nearly one v row (|v| up to
    4.5 sigma), and that row's 22-bit limb image alone is off by 2^-23 |v|: with v at twice the scale the two-image kernel measured 2.50e-6 of
    the scale on counts (65, 63, 129, 2) at scale 40 (1.85e-6 at scale 1) -- the same bits as the existing entry gives for that scene alone
    (the bit-for-bit test above), i.e. the existing kernel's error on a 2 sigma operand, not something the counts add."""
    B, N, M, counts = case
    q, k = _rand(B, N, D, seed=51) * scale, _rand(B, M, D, seed=52) * scale
    v = k if kind == "ctx" else _rand(B, M, D, seed=53) * scale
    sm = 0.125 / (scale * scale)
    ref = _fp64(q, k, v, sm, counts)
    with _kernels() as kn:
        y = _attend(kind, q.to(DEV), k.to(DEV), v.to(DEV), sm, _cnt(counts)).cpu()
    assert kn.ran(_expected_kernel(kind, D, 1)), kn.launches
    err = (y.double() - ref).abs().max().item() / scale
    print(f"{kind} D {D} counts {counts} operand scale {scale}: max |y - fp64| / scale = {err:.2e}")
    assert err < 2e-6


@pytest.mark.parametrize("fp16", [1, 0])
@pytest.mark.parametrize("D,case", [(64, LIMB_CASES[0]), (64, LIMB_CASES[1]), (32, LIMB_CASES[0]), (32, LIMB_CASES[1]), (64, FP32_CASE), (128, FP32_CASE),
                                    (256, FP32_CASE)])
def test_op_attention_with_counts_against_fp64(D, case, fp16):
    """5e-6 under either setting of knob 5, operands drawn as test_gpu_ops.py::test_attention_matches_fp64 draws them: that file's _rand is
    UNIFORM on [-scale, scale] (q and k at 2, v at 1), not normal."""
    B, N, M, counts = case
    q, k, v = _uniform(B, N, D, seed=1, scale=2.0), _uniform(B, M, D, seed=2, scale=2.0), _uniform(B, M, D, seed=3)
    sm = D ** -0.5
    ref = _fp64(q, k, v, sm, counts)
    with knobs({5: fp16}):
        with _kernels() as kn:
            y = engine.op_attention(q.to(DEV), k.to(DEV), v.to(DEV), sm, counts=_cnt(counts)).cpu().double()
    assert kn.ran(_expected_kernel("kv", D, fp16)), kn.launches
    err = (y - ref).abs().max().item()
    print(f"op_attention D {D} counts {counts} knob 5 = {fp16}: max |y - fp64| = {err:.2e}")
    assert err < 5e-6


# ------------------------------------------------------------------ 3. counts all equal to M; 4. pad rows do not matter (operators)
@pytest.mark.parametrize("kind,fp16,D,case", OPERATOR_CASES)
def test_operator_full_counts_and_pad_rows(kind, fp16, D, case):
    """Counts all M give the bytes of the call without counts.  With rows >= count_b of k / v / c filled with NaN, and again with 1e30, the
    output is that with zeros bit for bit and no pass is repeated on the fp32 kernel (fc_debug_fp16_fallbacks does not move)."""
    lib = engine.lib()
    B, N, M, counts = case
    q, k, v = _rand(B, N, D, seed=81).to(DEV), _rand(B, M, D, seed=82, scale=2.0).to(DEV), _rand(B, M, D, seed=83).to(DEV)
    sm = D ** -0.5
    pad = torch.arange(M, device=DEV)[None, :, None] >= _cnt(counts)[:, None, None]
    with knobs({5: fp16}):
        assert torch.equal(_attend(kind, q, k, v, sm, _cnt([M] * B)), _attend(kind, q, k, v, sm))
        before = lib.fc_debug_fp16_fallbacks()
        zeros = _attend(kind, q, k.masked_fill(pad, 0.0), v.masked_fill(pad, 0.0), sm, _cnt(counts))
        for fill in (float("nan"), 1e30):
            y = _attend(kind, q, k.masked_fill(pad, fill), v.masked_fill(pad, fill), sm, _cnt(counts))
            assert torch.isfinite(y).all() and torch.equal(y, zeros), (kind, fp16, D, fill)
        assert lib.fc_debug_fp16_fallbacks() == before


# ------------------------------------------------------------------ 5. the engine
@functools.lru_cache(maxsize=None)
def _stack(name, device=DEV, N=130):
    """Two layers of a named configuration, built like _c2_stack of tests/test_gpu_attention_fold.py"""
    cfg = fa.named_config(name, n_flow_layers=2, sample_size=N)
    torch.manual_seed(7)
    md = fa.initialize_flow(cfg, device=device, mode="test")
    return cfg, md


def _engine_inputs(cfg, md, B=4, N=130, M=200, seed=91):
    """(x, context of random embeddings, extra [B, N, X] or None, pinned eps) on the CPU"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, N, cfg["input_dim"], generator=g)
    ctx = torch.randn(B, M, cfg["input_embedding_dim"], generator=g)
    extra = (torch.rand(B, 1, generator=g) * 15)[:, None, :].expand(-1, N, -1).contiguous() if cfg["using_extra_context"] else None
    eps = [torch.randn(s, generator=g) for s in md["flow"].noise_shapes(B, N)]
    return x, ctx, extra, eps


def _scene(b, c, x, ctx, extra, eps):
    """scene b alone with its first c context rows"""
    return x[b:b + 1], ctx[b:b + 1, :c], None if extra is None else extra[b:b + 1], [e[b:b + 1] for e in eps]


def _to(dev, x, ctx, extra, eps):
    return x.to(dev), ctx.to(dev), None if extra is None else extra.to(dev), [e.to(dev) for e in eps]


@contextlib.contextmanager
def _setting(setting, md):
    """"shipped", "fold0" (knob 33 = 0 when the engine is created: the stacked K|V projection and the two-image kernel) or "fp32" (knob 5 = 0);
    the module's engine handle is dropped on the way in and out so that the setting is the one packed"""
    try:
        with knobs({"shipped": {}, "fold0": {33: 0}, "fp32": {5: 0}}[setting]):
            md["flow"]._handle = None
            yield
    finally:
        md["flow"]._handle = None


SETTING_KERNEL = {"shipped": SHARED, "fold0": "attn16_kernel<64>", "fp32": "attn_kernel<64>"}


@pytest.mark.parametrize("setting", ["shipped", "fold0", "fp32"])
@pytest.mark.parametrize("name", ["c2_dgcnn_attn_spline", "c4_dgcnn_attn_extra_affine"])
def test_flow_log_prob_with_counts_equals_every_scene_alone(name, setting):
    """Flow.log_prob(..., context_counts)[b] against Flow.log_prob of scene b alone on context[b:b+1, :count_b].  First, through the existing
    path only, whether the uniform engine is batch-invariant on this fixture (the B-scene call against its B = 1 calls): where it is, the
    ragged comparison is torch.equal; where it is not, the ragged call may be no further from the scenes alone than the uniform call is.
    Then every scene against the fp64 oracle on its truncated context, at the gate of test_c2_layer_stack_fold_on_against_fold_off."""
    cfg, md = _stack(name)
    flow = md["flow"]
    cpu = _engine_inputs(cfg, md)
    x, ctx, extra, eps = _to(DEV, *cpu)
    B, M = ctx.shape[:2]
    counts = _cnt(ENGINE_COUNTS)
    sd_f = {k: v.cpu().double() for k, v in flow.state_dict().items()}
    with _setting(setting, md), torch.no_grad():
        uniform = flow.log_prob(x, context=ctx, extra_context=extra, eps=eps)
        uni_gap = max((uniform[b:b + 1] - flow.log_prob(xs, context=cs, extra_context=es, eps=ns)).abs().max().item()
                      for b in range(B) for xs, cs, es, ns in [_scene(b, M, x, ctx, extra, eps)])
        with _kernels() as kn:
            ragged = flow.log_prob(x, context=ctx, extra_context=extra, eps=eps, context_counts=counts)
        assert kn.ran(SETTING_KERNEL[setting]) and kn.ran("zero_pad_rows_kernel"), kn.launches
        assert torch.equal(flow.log_prob(x, context=ctx, extra_context=extra, eps=eps, context_counts=_cnt([M] * B)), uniform)      # (item 3)
        alone = [flow.log_prob(xs, context=cs, extra_context=es, eps=ns)
                 for xs, cs, es, ns in (_scene(b, c, x, ctx, extra, eps) for b, c in enumerate(ENGINE_COUNTS))]
    rag_gap = max((ragged[b:b + 1] - alone[b]).abs().max().item() for b in range(B))
    print(f"{name} [{setting}]: uniform batch against its scenes alone max |d| {uni_gap:.2e}; ragged batch against its scenes alone {rag_gap:.2e}")
    assert torch.isfinite(ragged).all()
    if uni_gap == 0.0:
        for b in range(B):
            assert torch.equal(ragged[b:b + 1], alone[b]), (name, setting, b)
    else:
        assert rag_gap <= uni_gap
    for b, c in enumerate(ENGINE_COUNTS):
        xs, cs, es, ns = _scene(b, c, *cpu)
        with torch.no_grad():
            lp_o = O.flow_log_prob(cfg, sd_f, xs.double(), cs.double(), None if es is None else es.double(), [e.double() for e in ns])
        d = (ragged[b:b + 1].cpu().double() - lp_o).abs().max().item()
        print(f"  scene {b} ({c} context points): max |log-prob - fp64 oracle| {d:.2e}")
        assert d < PER_POINT_TOL


@pytest.mark.parametrize("setting", ["shipped", "fold0", "fp32"])
def test_flow_log_prob_ignores_what_pad_rows_of_the_context_hold(setting):
    """Item 4 at the engine: context rows >= count_b filled with NaN, and with 1e30, give the bits of zeros there; no pass is repeated."""
    lib = engine.lib()
    cfg, md = _stack("c2_dgcnn_attn_spline")
    x, ctx, extra, eps = _to(DEV, *_engine_inputs(cfg, md))
    counts = _cnt(ENGINE_COUNTS)
    pad = torch.arange(ctx.shape[1], device=DEV)[None, :, None] >= counts[:, None, None]
    with _setting(setting, md), torch.no_grad():
        zeros = md["flow"].log_prob(x, context=ctx.masked_fill(pad, 0.0), eps=eps, context_counts=counts)
        assert torch.equal(zeros, md["flow"].log_prob(x, context=ctx, eps=eps, context_counts=counts))
        before = lib.fc_debug_fp16_fallbacks()
        for fill in (float("nan"), 1e30):
            lp = md["flow"].log_prob(x, context=ctx.masked_fill(pad, fill), eps=eps, context_counts=counts)
            assert torch.isfinite(lp).all() and torch.equal(lp, zeros), (setting, fill)
        assert lib.fc_debug_fp16_fallbacks() == before


# ------------------------------------------------------------------ 6. the probes
@pytest.mark.parametrize("setting", ["shipped", "fold0", "fp32"])
def test_attention_weights_and_mass_with_counts(setting):
    """Rows of scene b equal the single-scene call on columns < count_b, are exactly 0 beyond and sum to 1 within M 2^-23 (the tolerance of
    tests/test_gpu_attention_weights.py); masses likewise, with float weights and with None, each row summing to the sum of its weights
    within (M 2^-23 + (N + 4) 2^-24) sum |g| (tests/test_gpu_attention_mass.py)."""
    cfg, md = _stack("c2_dgcnn_attn_spline")
    flow = md["flow"]
    x, ctx, extra, eps = _to(DEV, *_engine_inputs(cfg, md))
    B, N, M = x.shape[0], x.shape[1], ctx.shape[1]
    counts, layers = _cnt(ENGINE_COUNTS), ("aug", 0, 1)
    idx = torch.tensor([0, 5, 64, 129, 17], device=DEV)
    g = torch.rand(B, N, generator=torch.Generator().manual_seed(5)).to(DEV) - 0.25
    with _setting(setting, md):
        with _kernels() as kn:
            ws = flow.attention_weights(x, context=ctx, layers=layers, points=idx, eps=eps, context_counts=counts)
        assert kn.ran("attn_weights_counts_kernel<64") and not kn.ran("attn_weights_kernel<"), kn.launches
        masses = {wt: flow.attention_mass(x, context=ctx, layers=layers, weights=wv, eps=eps, context_counts=counts) for wt, wv in (("g", g), ("ones", None))}
        for b, c in enumerate(ENGINE_COUNTS):
            xs, cs, _, ns = _scene(b, c, x, ctx, extra, eps)
            ws1 = flow.attention_weights(xs, context=cs, layers=layers, points=idx, eps=ns)
            for w, w1 in zip(ws, ws1):
                assert tuple(w.shape) == (B, idx.numel(), M)
                assert torch.equal(w[b:b + 1, :, :c], w1) and (w[b, :, c:] == 0).all(), (setting, b)
                assert (w[b].double().sum(-1) - 1.0).abs().max().item() <= M * 2.0 ** -23
            for wt, wv in (("g", g), ("ones", None)):
                ms1 = flow.attention_mass(xs, context=cs, layers=layers, weights=None if wv is None else wv[b:b + 1], eps=ns)
                gb = (g[b] if wv is not None else torch.ones(N, device=DEV)).double()
                for m, m1 in zip(masses[wt], ms1):
                    assert tuple(m.shape) == (B, M)
                    assert torch.equal(m[b:b + 1, :c], m1) and (m[b, c:] == 0).all(), (setting, wt, b)
                    assert abs(m[b].double().sum().item() - gb.sum().item()) <= (M * 2.0 ** -23 + (N + 4) * 2.0 ** -24) * gb.abs().sum().item()


# ------------------------------------------------------------------ 7. inner_loop with the DGCNN embedder
def test_inner_loop_with_counts_and_pad_context_batch():
    cfg, md = _stack("c2_dgcnn_attn_spline")
    kn_ = cfg["n_neighbors"]
    counts = (200, 137, 64, kn_)
    g = torch.Generator().manual_seed(11)
    clouds = [torch.rand(c, 6, generator=g).to(DEV) for c in counts]
    e1 = torch.rand(4, 130, 6, generator=g).to(DEV)
    eps = [torch.randn(s, generator=g).to(DEV) for s in md["flow"].noise_shapes(4, 130)]
    e0, cnt = fa.pad_context_batch(clouds)
    assert tuple(e0.shape) == (4, 200, 6) and cnt.dtype == torch.int32 and cnt.tolist() == list(counts)
    for b, c in enumerate(counts):
        assert torch.equal(e0[b, :c], clouds[b]) and (e0[b, c:] == 0).all()
    full = torch.rand(4, 200, 6, generator=g).to(DEV)                                    # a uniform batch: is inner_loop batch-invariant here?
    with torch.no_grad():
        _, lp_u, _ = fa.inner_loop((full, e1, None), md, cfg, eps=eps)
        uni_gap = max((lp_u[b:b + 1] - fa.inner_loop((full[b:b + 1], e1[b:b + 1], None), md, cfg, eps=[e[b:b + 1] for e in eps])[1]).abs().max().item() for b in range(4))
        loss, lp, bpd = fa.inner_loop((e0, e1, None), md, cfg, eps=eps, context_counts=cnt)
        alone = [fa.inner_loop((clouds[b][None], e1[b:b + 1], None), md, cfg, eps=[e[b:b + 1] for e in eps])[1] for b in range(4)]
    rag_gap = max((lp[b:b + 1] - alone[b]).abs().max().item() for b in range(4))
    print(f"inner_loop: uniform batch against its scenes alone max |d| {uni_gap:.2e}; ragged batch against its scenes alone {rag_gap:.2e}")
    if uni_gap == 0.0:
        assert torch.equal(lp, torch.cat(alone))
    else:
        assert rag_gap <= uni_gap
    cat = torch.cat(alone) if uni_gap == 0.0 else lp                                   # loss and bpd are those of the concatenated log-probs
    assert tuple(lp.shape) == (4, 130) and torch.equal(loss, -cat.mean())
    assert torch.equal(bpd, -cat.mean() * math.log2(math.exp(1)) / cfg["input_dim"])


# ------------------------------------------------------------------ 8. refusals
def test_refusals_by_their_messages():
    cfg, md = _stack("c2_dgcnn_attn_spline")
    flow = md["flow"]
    x, ctx, extra, eps = _to(DEV, *_engine_inputs(cfg, md))
    B, M = ctx.shape[:2]
    ok = list(ENGINE_COUNTS)
    for bad, message in ((_cnt([0] + ok[1:]), rf"context_counts out of range: count 0 is not in \[1, {M}\]"),
                         (_cnt(ok[:-1] + [M + 1]), rf"context_counts out of range: count {M + 1} is not in \[1, {M}\]"),
                         (_cnt(ok).float(), r"context_counts must be an integer tensor, got dtype torch.float32"),
                         (_cnt(ok).cpu(), r"context_counts must live on a HIP device \(there is no CPU path\), got a tensor on cpu"),
                         (_cnt(ok + [5]), rf"context_counts must have shape \[B\] with B = {B} \(one count per scene\), got \({B + 1},\)")):
        with pytest.raises(RuntimeError, match=message):
            flow.log_prob(x, context=ctx, eps=eps, context_counts=bad)
        with pytest.raises(RuntimeError, match=message):
            fa.inner_loop((torch.rand(B, M, 6, device=DEV), x, None), md, cfg, eps=eps, context_counts=bad)
        with pytest.raises(RuntimeError, match=message.replace("context_counts", "counts")):
            engine.op_attention_ctx(ctx[:, :64], ctx, 0.125, counts=bad)
    # train mode
    flow.train()
    try:
        with pytest.raises(RuntimeError, match=r"Flow.log_prob: context_counts is eval-mode only \(the training path has no per-scene context point counts\)"):
            flow.log_prob(x, context=ctx, eps=eps, context_counts=_cnt(ok))
        with pytest.raises(RuntimeError, match=r"inner_loop: context_counts is eval-mode only"):
            fa.inner_loop((torch.rand(B, M, 6, device=DEV), x, None), md, cfg, eps=eps, context_counts=_cnt(ok))
    finally:
        flow.eval()
    # the global configuration
    cfg_g = fa.named_config("c1_dgcnn_global_affine", n_flow_layers=2, sample_size=130)
    md_g = fa.initialize_flow(cfg_g, device=DEV, mode="test")
    batch_g = (torch.rand(B, M, 6, device=DEV), torch.rand(B, 130, 6, device=DEV), None)
    with pytest.raises(RuntimeError, match=r"inner_loop: context_counts has no meaning with config\['global'\]"):
        fa.inner_loop(batch_g, md_g, cfg_g, context_counts=_cnt(ok))
    xg, ctx_g = batch_g[1][:, :, :cfg_g["input_dim"]], torch.rand(B, 130, cfg_g["input_embedding_dim"], device=DEV)
    with pytest.raises(RuntimeError, match=r"Flow.log_prob: context_counts has no meaning with config\['global'\]"):
        md_g["flow"].log_prob(xg, context=ctx_g, context_counts=_cnt([130] * B))
    with pytest.raises(engine.FcError, match=r"fc_flow_logprob_counts_f32: this flow has a global context"):       # the library's own refusal, behind the binding's
        h = md_g["flow"]._engine()
        h.is_global = False
        try:
            h.log_prob(xg, ctx_g, None, [torch.randn(s, device=DEV) for s in md_g["flow"].noise_shapes(B, 130)], context_counts=_cnt([130] * B))
        finally:
            h.is_global = True
    # a DGCNN count below n_neighbors: the embedder's own message
    below = _cnt(ok[:-1] + [cfg["n_neighbors"] - 1])
    with pytest.raises(engine.FcError, match="fewer context points than n_neighbors"):
        fa.inner_loop((torch.rand(B, M, 6, device=DEV), x, None), md, cfg, eps=eps, context_counts=below)
