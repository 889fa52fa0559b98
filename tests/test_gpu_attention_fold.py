"""The K|V fold of the inference engine on the GPU (csrc/flow_pack.cpp build_attn, csrc/flow_engine.cpp prepare, csrc/attention.hip attn16_kernel<64, 1>;
DESIGN.md sections 4, 5, 9): to_kv folded into the q projections and the consumers' in_layers, every attention attending over ONE limb
image of the context panel, a 64-key tile staged once for the S and the PV phase.  fc_debug_set key 33 (read when a flow is created)
selects the folded (1, shipped) or the projected-K|V engine (0); a test that flips it drops the module's engine handle so that the next
call packs a fresh one.  Which kernels ran is read from the in-library profiler, never assumed."""
import contextlib
import ctypes

import pytest
import torch

import attn_weights_util as U
import flowcompare_amd as fa
from flowcompare_amd import engine
from knob_util import knobs
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BPD_TOL = 1e-4                   # the project's gates against the fp64 oracle (tests/test_gpu_flow.py)
PER_POINT_TOL = 2e-3
SHARED = "attn16_kernel<64, 1>"  # the shared-tile kernel; the two-image kernel reports as attn16_kernel<64>


class _kernels:
    """{kernel name: launches} of the launches inside the block"""

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


@contextlib.contextmanager
def _fold(value, *mds):
    """knob 33 = value for the engines created inside the block; `mds` lose their handles on the way in and out"""
    def drop():
        for md in mds:
            md["flow"]._handle = None

    try:
        with knobs({33: value}):
            drop()
            yield
    finally:
        drop()


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------ 1. the shared-tile kernel alone
@pytest.mark.parametrize("B,N,M,D", [(2, 300, 280, 64), (1, 4096, 4096, 64), (3, 300, 777, 64), (2, 1000, 1250, 64), (2, 130, 33, 64), (1, 256, 64, 32), (2, 700, 33, 32)])
@pytest.mark.parametrize("scale", [1.0, 40.0, 0.05])
def test_shared_tile_attention_against_fp64(B, N, M, D, scale):
    """softmax(q c^T s) c with ONE tensor c as keys and values (fc_debug_attention_ctx_f32, the folded engine's two launches): at head dim 64 the kernel that stages each
    64-key tile once, in XOR-swizzled 256-byte rows read by rows (S) and transposed (PV); at 32 the two-image kernel on one image.  M = 280 (the
    layer-stack test's), 4096, ragged last tiles (777, 1250, 33 = one partial tile), queries and the key / value tensor of order 1, 40 and 0.05
    as in test_gpu_ops.test_attention_one_accumulator_form_against_fp64, whose bound this is: 2e-6 of the operand scale."""
    q, c = _rand(B, N, D, seed=51) * scale, _rand(B, M, D, seed=52) * scale
    sm = 0.125 / (scale * scale)                                            # keeps the scores at the magnitude of the unit case
    ref = torch.softmax((q.double() @ c.double().transpose(1, 2)) * sm, -1) @ c.double()
    cd = c.to(DEV)
    with _kernels() as kn:
        y = engine.op_attention_ctx(q.to(DEV), cd, sm).cpu()
    assert kn.ran(SHARED) == (D == 64) and kn.ran("attn16_kernel<32>") == (D == 32) and not kn.ran("attn16_kernel<64>"), kn.launches
    err = (y.double() - ref).abs().max().item() / scale
    two = (engine.op_attention(q.to(DEV), cd, cd, sm).cpu().double() - ref).abs().max().item() / scale      # (the two-image kernel, for the record)
    print(f"B {B} N {N} M {M} D {D} operand scale {scale}: max |y - fp64| / scale = {err:.2e}   (two-image kernel on the same operands {two:.2e}; max |y| / scale {ref.abs().max().item() / scale:.2f})")
    assert err < 2e-6


def test_shared_tile_attention_equals_the_two_image_kernel_bit_for_bit():
    """Same MFMAs on the same operands in the same order, only the LDS addresses differ: keys = values through the two-image kernel
    (fc_op_attention_f32 with v = k) gives the same bits -- a wrong swizzle term on any row or chunk would not."""
    for B, N, M in ((2, 300, 280), (1, 513, 4096), (3, 100, 777)):
        q, c = _rand(B, N, 64, seed=61).to(DEV), _rand(B, M, 64, seed=62, scale=2.0).to(DEV)
        with _kernels() as kn:
            one = engine.op_attention_ctx(q, c, 0.0625)
            two = engine.op_attention(q, c, c, 0.0625)
        assert kn.ran(SHARED) and kn.ran("attn16_kernel<64>"), kn.launches
        assert torch.equal(one, two), (B, N, M)


# ------------------------------------------------------------------ 2. the engine, fold on against fold off
def _c2_stack(n_layers=4, N=300, **over):
    cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=n_layers, sample_size=N, **over)
    torch.manual_seed(7)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    return cfg, md


def _inputs(B, N, M, seed=8):
    g = torch.Generator().manual_seed(seed)
    e0, e1 = torch.rand(B, M, 6, generator=g), torch.rand(B, N, 6, generator=g)
    eps = [torch.randn(B, N, 294, generator=g)]
    return e0, e1, eps


def test_c2_layer_stack_fold_on_against_fold_off():
    """The C2 layer stack of test_gpu_flow.test_every_kernel_variant_in_the_library_agrees_on_the_c2_layer_stack (4 layers, N = 300, M = 280)
    with knob 33 = 1 against 33 = 0: the bound that test gives every other arithmetic, < 5e-4 on the log-probs.  The folded run launches no
    K|V projection (one GEMM launch fewer, counted over all GEMM kernels: the tile size depends on the problem) and runs the shared-tile kernel."""
    cfg, md = _c2_stack()
    e0, e1, eps = _inputs(2, 300, 280)
    batch, eps_d = (e0.to(DEV), e1.to(DEV), None), [e.to(DEV) for e in eps]
    out, kernels = {}, {}
    for fold in (1, 0):
        with _fold(fold, md):
            fa.inner_loop(batch, md, cfg, eps=eps_d)                  # (packs the engine outside the profiled call)
            with _kernels() as kn:
                out[fold] = fa.inner_loop(batch, md, cfg, eps=eps_d)[1]
            kernels[fold] = kn
    assert kernels[1].ran(SHARED) and not kernels[1].ran("attn16_kernel<64>"), kernels[1].launches
    assert kernels[0].ran("attn16_kernel<64>") and not kernels[0].ran(SHARED), kernels[0].launches
    gemms = {f: sum(n for k, n in kernels[f].launches.items() if "gemm_f32_kernel" in k) for f in (0, 1)}
    assert gemms[0] - gemms[1] == 1, (gemms, "the stacked K|V projection is one GEMM launch per forward")
    assert kernels[1].launches.get("fc::kv_limbs_kernel") == 1, kernels[1].launches      # one context image per forward
    err = (out[1] - out[0]).abs().max().item()
    print(f"C2 layer stack, K|V fold on vs off: max |log-prob difference| {err:.2e}")
    assert torch.isfinite(out[1]).all() and err < 5e-4
    # and against the fp64 oracle
    sd_f = {k: v.cpu().double() for k, v in md["flow"].state_dict().items()}
    sd_e = {k: v.cpu().double() for k, v in md["input_embedder"].state_dict().items()}
    with torch.no_grad():
        _, lp_o, _ = O.inner_loop(cfg, sd_f, sd_e, (e0.double(), e1.double(), None), [e.double() for e in eps])
    for fold in (1, 0):
        d = (out[fold].cpu().double() - lp_o).abs().max().item()
        print(f"  fold {fold}: max |log-prob - fp64 oracle| {d:.2e}")
        assert d < PER_POINT_TOL


def test_sub_batch_of_two_scenes_reproduces_its_rows_bit_for_bit():
    """Scenes do not interact: scenes 1-2 of a 4-scene batch alone give the bits they had inside the batch (one context image for the whole
    batch, a scene's rows at other offsets of it)."""
    cfg, md = _c2_stack()
    e0, e1, eps = _inputs(4, 300, 280, seed=18)
    e0, e1, eps = e0.to(DEV), e1.to(DEV), [e.to(DEV) for e in eps]
    with _kernels() as kn:
        _, full, _ = fa.inner_loop((e0, e1, None), md, cfg, eps=eps)
    assert kn.ran(SHARED), kn.launches
    _, sub, _ = fa.inner_loop((e0[1:3], e1[1:3], None), md, cfg, eps=[eps[0][1:3]])
    assert torch.equal(sub, full[1:3])


def test_parameter_change_refolds_to_kv():
    """A changed to_kv weight must reach the folded q projection and in_layer on the next call (the re-pack), and restoring it must give the
    first bits again."""
    cfg, md = _c2_stack()
    e0, e1, eps = _inputs(2, 300, 280, seed=28)
    batch, eps = (e0.to(DEV), e1.to(DEV), None), [e.to(DEV) for e in eps]
    _, lp0, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    w = md["flow"].transforms[4].pre_conditioner.attn.fn.attention.to_kv.weight
    for row in (3, 64 + 3):                                            # a K row, then a V row
        with torch.no_grad():
            saved = w[row].clone()
            w[row] += 0.5
        _, lp1, _ = fa.inner_loop(batch, md, cfg, eps=eps)
        assert not torch.equal(lp0, lp1), row
        with torch.no_grad():
            w[row] = saved
        _, lp2, _ = fa.inner_loop(batch, md, cfg, eps=eps)
        assert torch.equal(lp0, lp2), row


def test_out_of_range_context_repeats_on_the_bf16_limbs_and_still_matches():
    """A context value beyond the one-accumulator image's range (|x| 16 >= 65504) raises the range flag where the K|V projection's epilogue
    raised it -- in the context-image pass -- and the whole forward repeats on the bf16-limb GEMMs with the fp32-input attention over the fp32
    panel.  The value (5000, on one context point of scene 0) sits in an embedding column that every to_kv ignores (its weight column is
    zeroed), so that the flow itself stays where fp32 can follow it -- in a live column the value enters the softmax-weighted means and with
    them the coupling nets, and scene 0's log-probs are no longer finite -- while the image still cannot hold it.  Against the fp64 oracle on the same context and
    weights, at the project's per-point gate."""
    lib = engine.lib()
    cfg, md = _c2_stack(n_layers=3)
    e0, e1, eps = _inputs(2, 300, 280, seed=38)
    with torch.no_grad():
        for name, prm in md["flow"].named_parameters():
            if name.endswith(".attention.to_kv.weight"):
                prm[:, 5] = 0.0
        emb = md["input_embedder"](e0.to(DEV)).clone()
    emb[0, 17, 5] = 5000.0
    x, eps_d = e1.to(DEV), [e.to(DEV) for e in eps]
    before = lib.fc_debug_fp16_fallbacks()
    with _kernels() as kn:
        lp = md["flow"].log_prob(x, context=emb, eps=eps_d)
    assert lib.fc_debug_fp16_fallbacks() == before + 1, "the pass was expected to repeat on the bf16 limbs"
    assert kn.ran(SHARED) and kn.ran("attn_kernel<64>"), kn.launches                      # the fast pass, then its repeat
    sd_f = {k: v.cpu().double() for k, v in md["flow"].state_dict().items()}
    with torch.no_grad():
        lp_o = O.flow_log_prob(cfg, sd_f, e1.double(), emb.cpu().double(), None, [e.double() for e in eps])
    d = (lp.cpu().double() - lp_o).abs()
    print(f"out-of-range context (bf16-limb repeat): max |log-prob - fp64 oracle| {d.max().item():.2e}  (scene 0 {d[0].max().item():.2e}, scene 1 {d[1].max().item():.2e})")
    assert torch.isfinite(lp).all() and d.max().item() < PER_POINT_TOL


# ------------------------------------------------------------------ 3. the attention-weights export
@pytest.mark.parametrize("case", [c for c in U.CASES if c != "e2e_tiny_cif"])
def test_exported_weights_with_the_fold_meet_the_reference_gate(case):
    """The fixtures of tests/test_gpu_attention_weights.py at the real widths (embedding 64 = inner 64: folded), same gate: max |w - w64| <=
    4 x E with both terms of E from the reference's own fp32 run.  The probe reads the context image and the folded q; the forward beside it
    runs the shared-tile kernel.  With knob 33 = 0 the same fixtures pass the same gate on the projected K (the two engines agree on what a
    weight is)."""
    fx, ref = U.load_case(case)
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    sd_flow, sd_emb = U.state_dicts(fx)
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    batch = tuple(None if t is None else t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
    eps = [e.to(DEV) for e in fx.eps()]
    layers = [U.layer_of(cfg, p) for p in ref.prefixes]
    for fold in (1, 0):
        with _fold(fold, md):
            with _kernels() as kn:
                ws = fa.attention_weights(batch, md, cfg, layers=layers, eps=eps)
        assert kn.ran(SHARED) == (fold == 1) and kn.ran("attn_weights_kernel<64, 1>"), kn.launches
        for i, w in enumerate(ws):
            w64, w32 = torch.as_tensor(ref.w64[i]).double(), torch.as_tensor(ref.w32[i]).double()
            err, bound = (w.double().cpu() - w64).abs().max().item(), U.gate((w32 - w64).abs().max().item(), w64.max().item())
            print(f"{case} fold {fold} attention {i} ({layers[i]}): max |w - fp64| {err:.2e}  ratio to E {4.0 * err / bound:.2f}  (gate 4)")
            assert tuple(w.shape) == tuple(w64.shape) and err <= bound, (case, fold, i)


# ------------------------------------------------------------------ 4. the gate's other side, the workspace
@pytest.mark.parametrize("E", [32, 128])
def test_other_embedding_widths_take_the_projected_path_and_match_the_oracle(E):
    """input_embedding_dim 32 / 128 against an inner dimension of 64: the fold would change weight shapes, the gate refuses it, the stacked
    K|V projection and the two-image kernel run as before -- against the fp64 oracle at the project's gates."""
    cfg, md = _c2_stack(n_layers=2, N=200, input_embedding_dim=E)
    e0, e1, eps = _inputs(2, 200, 150, seed=48)
    with _kernels() as kn:
        _, lp, bpd = fa.inner_loop((e0.to(DEV), e1.to(DEV), None), md, cfg, eps=[e.to(DEV) for e in eps])
    assert kn.ran("attn16_kernel<64>") and not kn.ran(SHARED), kn.launches
    sd_f = {k: v.cpu().double() for k, v in md["flow"].state_dict().items()}
    sd_e = {k: v.cpu().double() for k, v in md["input_embedder"].state_dict().items()}
    assert sd_f["transforms.0.attn.fn.attention.to_kv.weight"].shape == (128, E)
    with torch.no_grad():
        _, lp_o, bpd_o = O.inner_loop(cfg, sd_f, sd_e, (e0.double(), e1.double(), None), [e.double() for e in eps])
    d = (lp.cpu().double() - lp_o).abs()
    print(f"embedding width {E}: max {d.max():.2e} mean {d.mean():.2e} bpd diff {abs(float(bpd) - float(bpd_o)):.2e}")
    assert abs(float(bpd) - float(bpd_o)) < BPD_TOL and d.max() < PER_POINT_TOL


def test_c2_workspace_shrinks_by_the_kv_region():
    """fc_flow_workspace_bytes at C2 (16 x 4096 + 4096 points, 115 layers + the augmenter = 116 attentions): the folded engine plans no K|V
    region -- 65536 rows x 116 x 128 limb-image columns x 4 B = 3.9 GB -- and one context image instead of a layer's two."""
    cfg, md = _c2_stack(n_layers=115, N=4096)
    need = {}
    for fold in (1, 0):
        with _fold(fold, md):
            h = md["flow"]._engine()
            n = ctypes.c_size_t()
            engine.lib().fc_flow_workspace_bytes(h._h, 16, 4096, 4096, ctypes.byref(n))
            need[fold] = n.value
    kv_region = 16 * 4096 * 116 * 128 * 4
    print(f"C2 workspace: {need[0] / 2**30:.2f} GiB with the K|V projection, {need[1] / 2**30:.2f} GiB folded (K|V region {kv_region / 2**30:.2f} GiB)")
    assert need[0] - need[1] >= kv_region
