"""End-to-end parity of the HIP engine behind the reference's module API (initialize_flow / inner_loop) against
(a) golden vectors produced by running the reference in fp64 and fp32 and (b) the pinned CPU oracle.

Tolerances (north_star: nats within 1e-4): the reference's own fp32 forward differs from its fp64
forward by up to ~8e-4 nats per point on these fixtures, so the 1e-4 gate is applied to the logged scalar
(bpd = mean nats * log2(e) / 6, what the reference logs as 'nats') against the fp64 golden, and per-point log-probs
must stay within PER_POINT_TOL of the fp64 golden (same order as the reference's own fp32 noise)."""
import numpy as np
import pytest
import torch

import flowcompare_amd as fa
from conftest import Fixture
from knob_util import knobs
from oracle import flow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BPD_TOL = 1e-4
PER_POINT_TOL = 2e-3
MEAN_ABS_TOL = 3e-4

SUPPORTED = ["e2e_dulcet_L3", "e2e_c1_global_L2", "e2e_spline_L2", "e2e_affine_exp_L2", "e2e_tiny_affine", "e2e_tiny_spline_relu",
             "e2e_tiny_random_permute", "e2e_tiny_FullCombiner", "e2e_tiny_ExponentialCombiner", "e2e_tiny_global_extra",
             "e2e_tiny_identity_aug", "e2e_tiny_cif", "e2e_tiny_expcoupling", "e2e_tiny_expcoupling_orig", "e2e_paconv_L2"]


def _build(fx):
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    sd_flow, sd_emb = fx.state_dicts()
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    return cfg, md


@pytest.mark.parametrize("name", SUPPORTED)
def test_inner_loop_matches_reference_golden(name):
    fx = Fixture(name)
    cfg, md = _build(fx)
    batch = tuple(None if t is None else t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
    eps = [e.to(DEV) for e in fx.eps()]
    loss, lp, bpd = fa.inner_loop(batch, md, cfg, eps=eps)
    lp = lp.cpu().double().numpy()
    d64 = np.abs(lp - fx.a["log_prob_f64"])
    print(f"{name}: vs fp64 golden max {d64.max():.2e} mean {d64.mean():.2e}; ref fp32 vs fp64 max "
          f"{np.abs(fx.a['log_prob_f32'] - fx.a['log_prob_f64']).max():.2e}; bpd diff {abs(float(bpd) - float(fx.a['bpd_f64'])):.2e}")
    assert np.isfinite(lp).all()
    assert abs(float(bpd) - float(fx.a["bpd_f64"])) < BPD_TOL
    assert abs(float(loss) - float(fx.a["loss_f64"])) < 6 * BPD_TOL / np.log2(np.e) * 1.0 + 1e-4
    assert d64.max() < PER_POINT_TOL and d64.mean() < MEAN_ABS_TOL


@pytest.mark.parametrize("name", SUPPORTED)
def test_embedder_and_latent_match_reference_golden(name):
    fx = Fixture(name)
    cfg, md = _build(fx)
    e0 = fx.t("extract_0").to(DEV)
    emb = md["input_embedder"](e0[:, :, :6])
    ref = fx.a["emb_f64"]
    d = np.abs(emb.cpu().double().numpy() - ref)
    print(f"{name}: embedder max {d.max():.2e} mean {d.mean():.2e}")
    assert d.mean() < 1e-5 and np.quantile(d, 0.99) < 1e-4        # k-NN near-ties may move a few points (max-pool is discontinuous)
    # latent after the last transform, from the engine's diagnostic output
    ctx = torch.from_numpy(ref).float().to(DEV)
    if ctx.dim() == 2:
        ctx = ctx[:, None, :].expand(-1, fx.meta["N"], -1)
    extra = fx.t("extra")
    extra = None if extra is None else extra.to(DEV)[:, None, :].expand(-1, fx.meta["N"], -1)
    lp, z = md["flow"]._engine().log_prob(fx.t("extract_1").to(DEV), ctx, extra, [e.to(DEV) for e in fx.eps()], return_latent=True)
    dz = np.abs(z[:, :8].cpu().double().numpy() - fx.a["z_last_f64"])
    print(f"{name}: latent max {dz.max():.2e}")
    assert dz.max() < 5e-4
    assert np.abs(lp.cpu().double().numpy() - fx.a["log_prob_f64"]).max() < PER_POINT_TOL


@pytest.mark.parametrize("name", SUPPORTED)
def test_make_sample_matches_reference_golden(name):
    """Inverse / sampling path (models/transform.py:79-84) from the fixture's fixed latent z, through make_sample."""
    fx = Fixture(name)
    cfg, md = _build(fx)

    class FixedZ:
        def sample(self, num_samples, n_points=None, context=None):
            return fx.t("sample_z").float().to(DEV)

    inv_eps = [e.to(DEV) for e in fx.eps(prefix="inveps")]
    md["flow"]._inverse_eps = inv_eps or None
    extra = fx.t("extra")
    x = fa.make_sample(24, fx.t("extract_0")[:1].to(DEV), md, cfg, sample_distrib=FixedZ(),
                       extra_context=None if extra is None else extra[:1].to(DEV))
    d = np.abs(x.cpu().double().numpy() - fx.a["sample_x_f64"])
    scale = max(1.0, float(np.abs(fx.a["sample_x_f64"]).max()))     # e2e_tiny_cif's random-weight inverse reaches |x| ~ 6e4
    print(f"{name}: sample max err {d.max():.2e} (|x|max {scale:.1f})")
    assert d.max() < 5e-4 * scale


def test_inverse_roundtrip_real_dims():
    """forward(inverse(z)) latent == z at the real dims (invertibility: free property of the domain)."""
    fx = Fixture("e2e_dulcet_L3")
    cfg, md = _build(fx)
    h = md["flow"]._engine()
    ctx = torch.from_numpy(fx.a["emb_f64"]).float().to(DEV)
    extra = fx.t("extra").to(DEV)
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(2, 64, 300, generator=g) * 0.6).to(DEV)
    x = h.inverse(z, ctx, extra, None)
    assert x.shape == (2, 64, 6) and torch.isfinite(x).all()
    # the augmenter discards 294 dims, so check invertibility on the transforms after it: log_prob's latent of x differs from z,
    # but inverse must be deterministic and finite; exact round trip is checked on the identity-augmenter fixture below
    fx2 = Fixture("e2e_tiny_identity_aug")
    cfg2, md2 = _build(fx2)
    h2 = md2["flow"]._engine()
    ctx2 = torch.from_numpy(fx2.a["emb_f64"]).float().to(DEV)
    z2 = (torch.randn(2, 20, 6, generator=g) * 0.6).to(DEV)
    x2 = h2.inverse(z2, ctx2[:, :24], None, None)
    _, zz = h2.log_prob(x2, ctx2[:, :24], None, [], return_latent=True)
    assert (zz - z2).abs().max().item() < 2e-4


def test_matches_oracle_on_fresh_seeded_inputs():
    """HIP path vs the pinned oracle on inputs no fixture contains (module-initialised weights, torch RNG)."""
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=4, sample_size=200)
    torch.manual_seed(3)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    g = torch.Generator().manual_seed(4)
    B, N, M = 3, 200, 333
    e0, e1, ex = torch.rand(B, M, 6, generator=g), torch.rand(B, N, 6, generator=g), torch.rand(B, 1, generator=g) * 15
    eps = [torch.randn(B, N, 294, generator=g)]
    loss, lp, bpd = fa.inner_loop((e0.to(DEV), e1.to(DEV), ex.to(DEV)), md, cfg, eps=[e.to(DEV) for e in eps])
    sd_f = {k: v.cpu().double() for k, v in md["flow"].state_dict().items()}
    sd_e = {k: v.cpu().double() for k, v in md["input_embedder"].state_dict().items()}
    with torch.no_grad():
        _, lp_o, bpd_o = O.inner_loop(cfg, sd_f, sd_e, (e0.double(), e1.double(), ex.double()), [e.double() for e in eps])
    d = (lp.cpu().double() - lp_o).abs()
    print(f"fresh inputs: max {d.max():.2e} mean {d.mean():.2e} bpd diff {abs(float(bpd) - float(bpd_o)):.2e}")
    assert abs(float(bpd) - float(bpd_o)) < BPD_TOL and d.max() < PER_POINT_TOL


def test_scene_independence_and_determinism():
    """Scenes are independent: running a sub-batch gives bit-identical log-probs; two runs are bit-identical."""
    fx = Fixture("e2e_dulcet_L3")
    cfg, md = _build(fx)
    batch = tuple(t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
    eps = [e.to(DEV) for e in fx.eps()]
    _, lp1, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    _, lp2, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    assert torch.equal(lp1, lp2)
    _, lp_b1, _ = fa.inner_loop(tuple(t[1:2] for t in batch), md, cfg, eps=[e[1:2] for e in eps])
    assert torch.equal(lp_b1[0], lp1[1])


def test_unsupported_and_bad_arguments_fail_loudly():
    fx = Fixture("e2e_tiny_affine")
    cfg, md = _build(fx)
    with pytest.raises(RuntimeError, match="extra"):
        md["flow"].log_prob(fx.t("extract_1").to(DEV), context=torch.zeros(3, 24, 10, device=DEV), extra_context=None)
    with pytest.raises(RuntimeError, match="n_neighbors|fewer"):
        md["input_embedder"](torch.rand(1, 5, 6, device=DEV))
    with pytest.raises(RuntimeError, match="noise"):
        md["flow"].log_prob(fx.t("extract_1").to(DEV), context=torch.zeros(3, 24, 10, device=DEV),
                            extra_context=torch.zeros(3, 20, 1, device=DEV), eps=[])


def test_out_of_fp16_range_activations_repeat_on_the_bf16_limb_path():
    """Hidden activations of ~1e6 do not fit the fp16 limbs: the forward raises its range flag, is repeated with the bf16-limb
    GEMMs, and still matches the reference golden.  A ReLU MLP is positively homogeneous, so scaling its
    in_layer and every hidden bias by alpha and its out_layer weight by 1/alpha leaves the flow unchanged while every hidden
    activation of that net grows by alpha."""
    from flowcompare_amd import engine
    lib = engine.lib()
    fx = Fixture("e2e_tiny_spline_relu")
    cfg = dict(fx.cfg)
    sd_flow, sd_emb = fx.state_dicts()
    batch = tuple(t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
    eps = [e.to(DEV) for e in fx.eps()]
    ref = torch.from_numpy(fx.a["log_prob_f64"])
    for alpha, expect_fallback in ((1.0, False), (1.0e6, True)):
        sd = {k: v.clone() for k, v in sd_flow.items()}
        pre = "transforms.4.transform.nn."
        for k in sd:
            if k.startswith(pre):
                if k.startswith(pre + "in_layer.") or (k.startswith(pre + "layers.") and k.endswith(".bias")):
                    sd[k] = sd[k] * alpha
                elif k == pre + "out_layer.weight":
                    sd[k] = sd[k] / alpha
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
        fa.load_flow({"flow": sd, "input_embedder": sd_emb}, md)
        before = lib.fc_debug_fp16_fallbacks()
        _, lp, bpd = fa.inner_loop(batch, md, cfg, eps=eps)
        assert (lib.fc_debug_fp16_fallbacks() > before) == expect_fallback
        err = (lp.cpu().double() - ref).abs().max().item()
        print(f"alpha {alpha:g}: fallback {expect_fallback}, max |log-prob - fp64 golden| {err:.2e}")
        assert torch.isfinite(lp).all() and err < PER_POINT_TOL and abs(float(bpd) - float(fx.a["bpd_f64"])) < BPD_TOL


def test_deferred_range_check_queues_forwards_back_to_back_and_still_repeats_out_of_range_passes():
    """fc_range_check_defer (include/fcflow.h): inside `engine.deferred_range_check()` the embedder and flow entry points only enqueue their
    fast pass (no stream synchronisation per call); the flags are read at resolve.  (i) Two forwards queued back to back equal the
    synchronously checked ones bit for bit and nothing is repeated; (ii) a pass that leaves fp16's range (the alpha = 1e6 ReLU net of the
    test above) is repeated at resolve on the bf16-limb loops, its output is rewritten in place and matches the golden."""
    from flowcompare_amd import engine
    lib = engine.lib()
    fx = Fixture("e2e_tiny_spline_relu")
    cfg = dict(fx.cfg)
    sd_flow, sd_emb = fx.state_dicts()
    batch = tuple(t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
    batch2 = (batch[0].flip(0).contiguous(), batch[1].flip(0).contiguous(), None if batch[2] is None else batch[2].flip(0).contiguous())
    eps = [e.to(DEV) for e in fx.eps()]
    eps2 = [e.flip(0).contiguous() for e in eps]
    ref = torch.from_numpy(fx.a["log_prob_f64"])
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    _, lp_a, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    _, lp_b, _ = fa.inner_loop(batch2, md, cfg, eps=eps2)
    with engine.deferred_range_check() as drc:
        _, q_a, _ = fa.inner_loop(batch, md, cfg, eps=eps)
        assert lib.fc_range_check_pending() == 2                  # embedder pass + flow pass, neither waited for
        _, q_b, _ = fa.inner_loop(batch2, md, cfg, eps=eps2)
        assert lib.fc_range_check_pending() == 4
    assert drc.repeated == 0 and lib.fc_range_check_pending() == 0
    assert torch.equal(q_a, lp_a) and torch.equal(q_b, lp_b)
    # (ii) out-of-range hidden activations
    sd = {k: v.clone() for k, v in sd_flow.items()}
    pre = "transforms.4.transform.nn."
    for k in sd:
        if k.startswith(pre + "in_layer.") or (k.startswith(pre + "layers.") and k.endswith(".bias")):
            sd[k] = sd[k] * 1.0e6
        elif k == pre + "out_layer.weight":
            sd[k] = sd[k] / 1.0e6
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    fa.load_flow({"flow": sd, "input_embedder": sd_emb}, md)
    before = lib.fc_debug_fp16_fallbacks()
    with engine.deferred_range_check() as drc:
        _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps)
        _, lp2, _ = fa.inner_loop(batch2, md, cfg, eps=eps2)
    torch.cuda.synchronize()
    assert drc.repeated >= 2 and lib.fc_debug_fp16_fallbacks() >= before + 2
    err = (lp.cpu().double() - ref).abs().max().item()
    err2 = (lp2.flip(0).cpu().double() - ref).abs().max().item()
    print(f"deferred check: {drc.repeated} passes repeated at resolve, max |log-prob - fp64 golden| {err:.2e} / {err2:.2e}")
    assert torch.isfinite(lp).all() and err < PER_POINT_TOL and err2 < PER_POINT_TOL


def test_every_kernel_variant_in_the_library_agrees_on_the_c2_layer_stack():
    """The shipped fast paths (split-fp16 GEMM on eight-wave tiles, fused spline epilogue, split-fp16 attention, row-resident chains)
    against the paths that stay in the library beside them -- the per-layer launches small batches take, the unfused spline of the inverse
    direction, the bf16-limb range fallback, the fp32-input reference loop: same log-probs within the fp32 noise of a 4-layer flow at the
    real layer widths, and bit-identical ones where the arithmetic is the same.  Every case runs: a refused knob value fails the test."""
    cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=4, sample_size=300)
    torch.manual_seed(7)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    g = torch.Generator().manual_seed(8)
    B, N, M = 2, 300, 280
    e0, e1 = torch.rand(B, M, 6, generator=g), torch.rand(B, N, 6, generator=g)
    eps = [torch.randn(B, N, 294, generator=g).to(DEV)]
    batch = (e0.to(DEV), e1.to(DEV), None)

    def run_with(settings):
        """log-probs under the given knob values"""
        with knobs(settings):
            return fa.inner_loop(batch, md, cfg, eps=eps)[1]

    _, ref, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    for name, settings in (("unfused spline", {7: 0}), ("separate pre-attention GEMM launches + LayerNorm -> q fold", {8: 0}), ("separate LayerNorm + q projection", {8: 0, 10: 0}), ("no limb chain", {9: 0}), ("limb chain into the spline GEMM only", {16: 0}), ("fp32-input attention", {5: 0}),
                        ("bf16-limb GEMM", {0: 3}), ("fp32-input MFMA GEMM", {0: 2})):
        lp = run_with(settings)
        err = (lp - ref).abs().max().item()
        print(f"{name}: max |log-prob - default path| {err:.2e}")
        assert err < 5e-4, name
    # the row-resident coupling-MLP chain (the engine takes it where a launch fills the chip; this batch is 3 row tiles: forced) issues the
    # same MFMAs in the same k order as the per-layer launches and adds bias, residual, GELU and limb split alike: bit-identical
    lp = run_with({23: 2})
    assert torch.equal(lp, ref), "the row-resident chain differs from the per-layer launches"
    lp = run_with({23: 2, 16: 0})
    assert (lp - ref).abs().max().item() < 5e-4
    # round 4: the shipped fused spline layer is the 256 x 256 one-accumulator kernel on 16x16x32 MFMAs (spline_wide.hip, knob 13 = 5): another
    # arithmetic (one fp32 accumulator, unscaled low limbs, k32 MFMAs) than the 128 x 128 loops beside it -- same log-probs within fp32 noise
    ref4 = run_with({13: 4})
    err = (ref4 - ref).abs().max().item()
    print(f"persistent 128x128 fused spline GEMM (knob 13 = 4): max |log-prob - default path| {err:.2e}")
    assert err < 5e-4
    # both main loops of the 128 x 128 family issue the same MFMAs in the same k order and hand the same parameters to the same
    # spline arithmetic: the LDS-DMA loop with the LDS parameter tile (2) and the persistent transposed product evaluated from the
    # accumulator registers (4) give bit-identical log-probs
    lp = run_with({13: 2})
    print(f"knob 13 = 2: max |diff| {(lp - ref4).abs().max().item():.3e}")
    assert torch.equal(lp, ref4), "fused spline GEMM variant (knob 13 = 2) differs from the persistent 128x128 loop"
    lp = run_with({22: 0})                                    # 128x128 tiles also for launches with few tiles (this test: 5 row tiles -> 64x64 tiles by default)
    assert torch.equal(lp, ref), "64x64 tiles for small launches changed the limb-chained GEMMs' results"


def test_persistent_spline_gemm_walks_several_tiles_per_workgroup():
    """Both fused spline kernels are persistent.  The shipped 256 x 256 one-accumulator kernel (spline_wide.hip, knob 13 = 5) runs one workgroup
    per CU over 256-row x 2-tile pairs with one continuous DMA stream: 19 row tiles x 15 pairs = 285 tiles > 256 slots on the plain tile
    order, 24 x 15 = 360 on the column-group order (row tiles a multiple of 8) -- a scene's log-probs must not depend on where its tiles fall
    (bit for bit the run of that scene alone, one tile per workgroup), and must agree with the 128 x 128 persistent loop (knob 13 = 4: two
    workgroups per CU, 18 x 30 = 540 / 24 x 30 = 720 tiles) within fp32 noise.  That loop in turn must come out exactly as the
    one-tile-per-workgroup kernel of its family (knob 13 = 2: the LDS-DMA loop with the LDS parameter tile)."""
    for B, N in ((3, 768), (3, 1000), (3, 1600), (3, 2048)):       # 2304 rows; 3000 rows + 72 padding rows; 4800 rows = 19 tiles of 256; 6144 = 24
        cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=2, sample_size=N)
        torch.manual_seed(21)
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
        with torch.no_grad():
            for name, prm in md["flow"].named_parameters():       # (module init zeroes nothing here, but make the parameter layer lively)
                if "out_layer" in name:
                    prm.mul_(3.0)
        g = torch.Generator().manual_seed(22)
        e0, e1 = torch.rand(B, 200, 6, generator=g), torch.rand(B, N, 6, generator=g)
        eps = [torch.randn(B, N, 294, generator=g).to(DEV)]
        batch = (e0.to(DEV), e1.to(DEV), None)
        _, ref, _ = fa.inner_loop(batch, md, cfg, eps=eps)
        _, again, _ = fa.inner_loop(batch, md, cfg, eps=eps)
        assert torch.equal(again, ref), f"{B} x {N}: the wide fused spline kernel is not deterministic"
        _, solo, _ = fa.inner_loop((batch[0][1:2], batch[1][1:2], None), md, cfg, eps=[eps[0][1:2]])
        assert torch.equal(solo[0], ref[1]), f"{B} x {N}: a scene's log-probs depend on the tiles it falls on (wide fused spline kernel)"
        with knobs({13: 4}):
            _, ref4, _ = fa.inner_loop(batch, md, cfg, eps=eps)
        err = (ref4 - ref).abs().max().item()
        print(f"{B} x {N}: wide kernel vs the 128 x 128 persistent loop: max |diff| {err:.2e}")
        assert err < 1e-3
        with knobs({13: 2}):
            _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps)
        assert torch.equal(lp, ref4), f"{B} x {N}: persistent fused spline GEMM differs from knob 13 = 2"
        assert torch.isfinite(ref).all()


@pytest.mark.parametrize("latent_dim, act", [(200, "GELU"), (300, "RELU"), (264, "ELU")])
def test_row_resident_pre_attention_kernel_other_widths_and_activations(latent_dim, act):
    """The shipped pre-attention chain kernel (activations in registers, csrc/premlp.hip) away from the C2 shape it is specialised for:
    x1 widths 100 / 150 / 132 columns (k padded to 128 / 160 / 160: the in_layer's k steps read at run time or compile time, weight
    rows of 32 / 40 sixteen-byte chunks with their two swizzle masks and piece-to-row maps) and the three activations the reference
    accepts, against the separate GEMM launches.  K_pad 128 and 160 are all this test reaches, and through three flow layers; the kernel alone
    against fp64 at every K_pad from 32 to 256, all five activation codes and odd row counts is tests/test_gpu_premlp.py."""
    cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=3, sample_size=300, latent_dim=latent_dim, coupling_block_nonlinearity=act)
    torch.manual_seed(31)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    g = torch.Generator().manual_seed(32)
    B, N, M = 2, 300, 310
    e0, e1 = torch.rand(B, M, 6, generator=g), torch.rand(B, N, 6, generator=g)
    eps = [torch.randn(*sh, generator=g).to(DEV) for sh in md["flow"].noise_shapes(B, N)]      # (a CIF block per layer when cif_latent_dim > latent_dim)
    batch = (e0.to(DEV), e1.to(DEV), None)
    _, lp, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    with knobs({8: 0}):
        _, ref, _ = fa.inner_loop(batch, md, cfg, eps=eps)
    err = (lp - ref).abs().max().item()
    print(f"latent {latent_dim}, {act}: max |row-resident - separate launches| {err:.2e}")
    assert torch.isfinite(lp).all() and err < 5e-4


def test_c2_layer_widths_with_ragged_sizes_match_the_oracle():
    """The shipped C2 fast paths (fused spline epilogue with its limb chain, LayerNorm -> q fold, K|V limb images, split-fp16
    attention) at the real layer widths but ragged sizes: rows not a multiple of any tile (3 x 333 targets), 77 context points
    (one partial key tile, k-NN with k = 40 of 77)."""
    cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=2, sample_size=333)
    torch.manual_seed(9)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    g = torch.Generator().manual_seed(10)
    B, N, M = 3, 333, 77
    e0, e1 = torch.rand(B, M, 6, generator=g), torch.rand(B, N, 6, generator=g)
    eps = [torch.randn(B, N, 294, generator=g)]
    loss, lp, bpd = fa.inner_loop((e0.to(DEV), e1.to(DEV), None), md, cfg, eps=[e.to(DEV) for e in eps])
    sd_f = {k: v.cpu().double() for k, v in md["flow"].state_dict().items()}
    sd_e = {k: v.cpu().double() for k, v in md["input_embedder"].state_dict().items()}
    with torch.no_grad():
        _, lp_o, bpd_o = O.inner_loop(cfg, sd_f, sd_e, (e0.double(), e1.double(), None), [e.double() for e in eps])
    d = (lp.cpu().double() - lp_o).abs()
    print(f"ragged C2: max {d.max():.2e} mean {d.mean():.2e} bpd diff {abs(float(bpd) - float(bpd_o)):.2e}")
    assert lp.shape == (B, N) and abs(float(bpd) - float(bpd_o)) < BPD_TOL and d.max() < PER_POINT_TOL


@pytest.mark.parametrize("bins", [4, 16])
def test_spline_bin_counts_other_than_eight_match_the_oracle(bins):
    """num_bins_spline 4 and 16 (models/spline_coupling.py:69-169): 13 / 49 parameters per transformed dim, 9 / 2 dims per 128-column tile in
    the dim-major column order (only K = 8 uses the register-slot order and the transposed kernels), evaluated in the GEMM epilogue
    through the LDS parameter tile and, with knob 7 = 0, by the stand-alone spline kernel -- both against the fp64 oracle."""
    cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=2, sample_size=200, num_bins_spline=bins)
    torch.manual_seed(41)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    g = torch.Generator().manual_seed(42)
    B, N, M = 2, 200, 150
    e0, e1 = torch.rand(B, M, 6, generator=g), torch.rand(B, N, 6, generator=g)
    eps = [torch.randn(B, N, 294, generator=g)]
    batch = (e0.to(DEV), e1.to(DEV), None)
    sd_f = {k: v.cpu().double() for k, v in md["flow"].state_dict().items()}
    sd_e = {k: v.cpu().double() for k, v in md["input_embedder"].state_dict().items()}
    with torch.no_grad():
        _, lp_o, bpd_o = O.inner_loop(cfg, sd_f, sd_e, (e0.double(), e1.double(), None), [e.double() for e in eps])
    for fused in (1, 0):
        with knobs({7: fused}):
            _, lp, bpd = fa.inner_loop(batch, md, cfg, eps=[e.to(DEV) for e in eps])
        d = (lp.cpu().double() - lp_o).abs()
        print(f"{bins} bins, fused spline {fused}: max {d.max():.2e} bpd diff {abs(float(bpd) - float(bpd_o)):.2e}")
        assert abs(float(bpd) - float(bpd_o)) < BPD_TOL and d.max() < PER_POINT_TOL


def test_cif_stack_at_real_layer_widths_matches_the_oracle():
    """CIFblock (augment -> conditional affine -> slice around the attention-conditioned coupling, models/cif_block.py:49-112) at the
    real layer widths (latent 300, CIF latent 364): the pair-packed epilogues on the eight-wave tile with slot-buffered log-dets,
    against the fp64 oracle on fresh inputs."""
    cfg = fa.named_config("c2_dgcnn_attn_spline", flow_type="AffineCoupling", n_flow_layers=2, sample_size=150, cif_latent_dim=364,
                          net_cif_dist_hidden_dims=[64, 64], affine_cif_hidden=[256, 256, 256])
    torch.manual_seed(13)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    g = torch.Generator().manual_seed(14)
    B, N, M = 2, 150, 160
    e0, e1 = torch.rand(B, M, 6, generator=g), torch.rand(B, N, 6, generator=g)
    eps = [torch.randn(*s, generator=g) for s in md["flow"].noise_shapes(B, N)]
    assert len(eps) == 3                                             # the outer augmenter + one per CIF block
    loss, lp, bpd = fa.inner_loop((e0.to(DEV), e1.to(DEV), None), md, cfg, eps=[e.to(DEV) for e in eps])
    sd_f = {k: v.cpu().double() for k, v in md["flow"].state_dict().items()}
    sd_e = {k: v.cpu().double() for k, v in md["input_embedder"].state_dict().items()}
    with torch.no_grad():
        _, lp_o, bpd_o = O.inner_loop(cfg, sd_f, sd_e, (e0.double(), e1.double(), None), [e.double() for e in eps])
    d = (lp.cpu().double() - lp_o).abs()
    print(f"CIF real widths: max {d.max():.2e} mean {d.mean():.2e} bpd diff {abs(float(bpd) - float(bpd_o)):.2e}")
    assert abs(float(bpd) - float(bpd_o)) < BPD_TOL and d.max() < PER_POINT_TOL
    # the tiles the range guard falls back to (bf16 limbs on the 128x320 tile, two column tiles -> atomics on the log-prob) and the
    # fp32-input MFMA variant run the same pair epilogues
    for name, v in (("bf16-limb GEMM", 3), ("fp32-input MFMA GEMM", 2)):
        with knobs({0: v}):
            _, lp_v, _ = fa.inner_loop((e0.to(DEV), e1.to(DEV), None), md, cfg, eps=[e.to(DEV) for e in eps])
        err = (lp_v.cpu().double() - lp_o).abs().max().item()
        print(f"CIF real widths, {name}: max {err:.2e}")
        assert err < PER_POINT_TOL, name
    # the inverse pass (Slice.inverse draws z2, then the affine_cif inverse epilogue) at the same widths, against the oracle's
    h = md["flow"]._engine()
    emb = md["input_embedder"](e0.to(DEV))
    z = torch.randn(B, N, 300, generator=g) * 0.5
    xr = h.inverse(z.to(DEV), emb, None, [e.to(DEV) for e in eps[1:]])
    with torch.no_grad():
        ctx_o = O.context_embed(cfg, sd_e, e0.double())
        x_o = O.flow_inverse(cfg, sd_f, z.double(), ctx_o, None, [e.double() for e in eps[1:]])
    rt = (xr.cpu().double() - x_o).abs().max().item() / max(1.0, x_o.abs().max().item())
    print(f"CIF real widths: inverse vs oracle, max relative to |x|max {rt:.2e}")
    assert rt < 5e-4


def test_parameter_change_triggers_a_fast_repack():
    """Evaluating between optimiser steps (train.py:134-170): any in-place parameter change re-packs the engine on the next call (folding on
    a pool of host threads, limb images made on the device).  The changed weight must take effect, restoring it must reproduce the
    first result bit for bit, and a re-pack of this 8-layer spline flow at the real widths must stay far below a second."""
    import time
    cfg = fa.named_config("c2_dgcnn_attn_spline", n_flow_layers=8, sample_size=200)
    torch.manual_seed(3)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    g = torch.Generator().manual_seed(4)
    e0, e1 = torch.rand(2, 256, 6, generator=g).to(DEV), torch.rand(2, 200, 6, generator=g).to(DEV)
    eps = [torch.randn(2, 200, 294, generator=g).to(DEV)]
    _, lp0, _ = fa.inner_loop((e0, e1, None), md, cfg, eps=eps)
    w = md["flow"].transforms[4].transform.nn.layers[0].weight
    with torch.no_grad():
        saved = w[3, 5].clone()
        w[3, 5] += 0.5
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, lp1, _ = fa.inner_loop((e0, e1, None), md, cfg, eps=eps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert not torch.equal(lp0, lp1)
    with torch.no_grad():
        w[3, 5] = saved
    _, lp2, _ = fa.inner_loop((e0, e1, None), md, cfg, eps=eps)
    assert torch.equal(lp0, lp2)
    print(f"re-pack + forward of an 8-layer spline flow after a parameter change: {dt * 1e3:.0f} ms")
    assert dt < 1.0
