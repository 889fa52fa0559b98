"""ExponentialCoupling beyond d2 = 16 (csrc/expm_wide.hip: the action of the per-point matrix exponential, Al-Mohy & Higham 2011):
reference parity on the fixtures of tests/golden/gen_golden_expm_wide.py, the operator against fp64 torch.matrix_exp over widths and norms,
the limits (d2 <= 256, the kernel's norm bound), the row chunking of the parameter panel, and a full-depth run at the reference's native
batch shape.  Gates of tests/test_gpu_flow.py."""
import time

import numpy as np
import pytest
import torch

import flowcompare_amd as fa
from conftest import Fixture
from flowcompare_amd import engine
from flowcompare_amd.conditioning import condition_flow
from fullsize_util import check_rows_against_fp64, oracle_flow_rows, side_by_side, synth_pairs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BPD_TOL, PER_POINT_TOL, MEAN_ABS_TOL, LATENT_TOL = 1e-4, 2e-3, 3e-4, 5e-4
EXPWIDE = ["e2e_expwide_d20", "e2e_expwide_d21_orig", "e2e_expwide_L2"]
CHUNK_D150 = 2048          # rows of the engine's parameter-panel chunk at d2 = 150 (flow_engine.cpp expm_chunk_rows: 192 MiB / 90 624 B)


def _build(fx):
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    sd_flow, sd_emb = fx.state_dicts()
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    return cfg, md


def expm_action(raw, x2, scal4, d2, inverse=False):
    """fc_op_expm_action_f32 on dense [P, d2*d2 + d2] / [P, d2] device tensors -> (y2, ldj, info [P, 4])."""
    P = raw.shape[0]
    y2 = torch.empty(P, d2, dtype=torch.float32, device=DEV)
    ldj = torch.empty(P, dtype=torch.float32, device=DEV)
    info = torch.empty(P, 4, dtype=torch.float32, device=DEV)
    engine.lib().fc_op_expm_action_f32(engine._ptr(raw), raw.shape[1], engine._ptr(x2), x2.shape[1], engine._ptr(scal4), engine._ptr(y2), d2,
                                       engine._ptr(ldj), engine._ptr(info), P, d2, int(inverse), engine._stream())
    return y2, ldj, info


# ------------------------------------------------------------------------------------------------ reference parity
@pytest.mark.parametrize("name", EXPWIDE)
def test_inner_loop_matches_reference_golden_at_wide_d2(name):
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
    assert d64.max() < PER_POINT_TOL and d64.mean() < MEAN_ABS_TOL
    ctx = torch.from_numpy(fx.a["emb_f64"]).float().to(DEV)
    extra = fx.t("extra")
    extra = None if extra is None else extra.to(DEV)[:, None, :].expand(-1, fx.meta["N"], -1)
    _, z = md["flow"]._engine().log_prob(fx.t("extract_1").to(DEV), ctx, extra, eps, return_latent=True)
    dz = np.abs(z[:, :8].cpu().double().numpy() - fx.a["z_last_f64"])
    print(f"{name}: latent max {dz.max():.2e}")
    assert dz.max() < LATENT_TOL


@pytest.mark.parametrize("name", EXPWIDE)
def test_make_sample_matches_reference_golden_at_wide_d2(name):
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
    scale = max(1.0, float(np.abs(fx.a["sample_x_f64"]).max()))
    print(f"{name}: sample max err {d.max():.2e} (|x|max {scale:.1f})")
    assert d.max() < 5e-4 * scale


# ------------------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize("d2", [17, 31, 32, 33, 64, 150, 255, 256])
def test_expm_action_against_fp64_matrix_exp(d2):
    P = 24
    g = torch.Generator().manual_seed(1000 + d2)
    raw = torch.randn(P, d2 * d2 + d2, generator=g)
    x2 = torch.randn(P, d2, generator=g)
    t = torch.tanh(raw[:, :d2 * d2].double()).view(P, d2, d2)
    base = t.abs().sum(1).amax(1)                        # ||tanh(raw)||_1 per point
    lines = []
    for target in (0.01, 0.5, 2.0, 8.0, 32.0):
        rescale = target / float(base.mean())
        scal4 = torch.tensor([1.0, 0.0, rescale, 0.0], dtype=torch.float32)
        w32 = rescale * torch.tanh(raw[:, :d2 * d2]).view(P, d2, d2) + 1e-8          # what torch does in fp32
        w64 = rescale * t + 1e-8
        b = raw[:, d2 * d2:]
        for inverse in (False, True):
            sgn = -1.0 if inverse else 1.0
            v64 = x2.double() - b.double() if inverse else x2.double()
            v32 = x2 - b if inverse else x2
            ref = torch.linalg.matrix_exp(sgn * w64) @ v64[..., None]
            ref32 = torch.linalg.matrix_exp(sgn * w32) @ v32[..., None]
            ref, ref32 = ref[..., 0], ref32[..., 0]
            if not inverse:
                ref, ref32 = ref + b.double(), ref32 + b
            y2, ldj, info = expm_action(raw.to(DEV), x2.to(DEV), scal4.to(DEV), d2, inverse)
            y2 = y2.cpu().double()
            scale = ref.abs().amax(1)
            err = ((y2 - ref).abs().amax(1) / scale)
            err32 = ((ref32.double() - ref).abs().amax(1) / scale)
            gate = torch.clamp(2 * err32, min=1e-4)
            info = info.cpu()
            lines.append(f"d2 {d2:3d} |W|1 {float(w64.abs().sum(1).amax(1).mean()):7.3f} {'inv' if inverse else 'fwd'}: rel err max {float(err.max()):.2e} "
                         f"(fp32 matrix_exp {float(err32.max()):.2e}); s {int(info[:, 1].max())} m {int(info[:, 2].max())} "
                         f"products mean {float(info[:, 3].mean()):.1f} max {int(info[:, 3].max())}")
            assert torch.isfinite(y2).all()
            assert bool((err <= gate).all()), lines[-1]
            # trace: the fp32 sum of the fp32 diagonal (exact up to fp32 summation and the tanh's rounding)
            diag = w64.diagonal(dim1=1, dim2=2)
            tol = 4 * d2 * 2.0 ** -24 * diag.abs().sum(1) + 1e-6
            assert bool(((ldj.cpu().double() - diag.sum(1)).abs() <= tol).all()), lines[-1]
    print("\n".join(lines))


def test_expm_action_limits():
    # d2 = 257: refused by the operator and by the engine at create, with a message that names the cap
    d2 = 257
    raw = torch.zeros(1, d2 * d2 + d2, device=DEV)
    x2 = torch.zeros(1, d2, device=DEV)
    scal4 = torch.tensor([1.0, 0.0, 1.0, 0.0], device=DEV)
    with pytest.raises(RuntimeError, match="256"):
        expm_action(raw, x2, scal4, d2)
    cfg = dict(Fixture("e2e_expwide_d20").cfg)
    cfg.update(latent_dim=514, cif_latent_dim=514, n_flow_layers=1)
    with pytest.raises(RuntimeError, match="ExponentialCoupling.*> 256"):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
        md["flow"]._engine()
    # a point beyond the kernel's norm bound: an error (host-side status), never a number
    d2 = 32
    g = torch.Generator().manual_seed(5)
    raw = torch.randn(4, d2 * d2 + d2, generator=g).to(DEV)
    x2 = torch.randn(4, d2, generator=g).to(DEV)
    for rescale in (40.0, float("nan")):
        with pytest.raises(RuntimeError, match="ExponentialCoupling"):
            expm_action(raw, x2, torch.tensor([1.0, 0.0, rescale, 0.0], device=DEV), d2)
    y2, _, _ = expm_action(raw, x2, torch.tensor([1.0, 0.0, 1.0, 0.0], device=DEV), d2)      # the stream is usable afterwards
    assert torch.isfinite(y2).all()


# ------------------------------------------------------------------------------------------------ chunking of the parameter panel
def test_chunk_boundaries_and_round_trip_at_d2_150():
    """The fixture's flow with its coupling matrices tamed (reshift 0, rescale / 4): the synthesised reshift of +-0.05 alone puts a
    rank-one eigenvalue of up to 7.5 into W at d2 = 150, and e^W e^-W then loses ~e^15 u of fp32 in any implementation -- this test is
    about the row chunks of the parameter panel, not about that conditioning."""
    fx = Fixture("e2e_expwide_L2")
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    sd_flow, sd_emb = fx.state_dicts()
    for k in sd_flow:
        if k.endswith("transform.reshift"):
            sd_flow[k] = torch.zeros_like(sd_flow[k])
        elif k.endswith("transform.rescale"):
            sd_flow[k] = sd_flow[k] * 0.25
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    h = md["flow"]._engine()
    ctx1 = torch.from_numpy(fx.a["emb_f64"]).float().to(DEV)
    ex1 = fx.t("extra")
    g = torch.Generator().manual_seed(7)
    solo = {}
    for B, N in ((1, CHUNK_D150 - 1), (1, CHUNK_D150 + 1), (3, 683)):         # P = chunk - 1, chunk + 1, and a ragged 3 x 683 = 2049
        x = torch.rand(B, N, 6, generator=g).to(DEV)
        eps = [torch.randn(B, N, 294, generator=g).to(DEV)]
        ctx = ctx1.expand(B, -1, -1).contiguous()
        extra = None if ex1 is None else ex1[:1].to(DEV)[:, None, :].expand(B, N, -1).contiguous()
        lp, z = h.log_prob(x, ctx, extra, eps, return_latent=True)
        assert torch.isfinite(lp).all() and torch.isfinite(z).all()
        # rows on both sides of every chunk boundary against the same rows computed alone (the points do not interact)
        for b, lo, hi in ((0, 0, 40), (B - 1, N - 40, N)):
            lpa = h.log_prob(x[b:b + 1, lo:hi].contiguous(), ctx[b:b + 1], None if extra is None else extra[b:b + 1, lo:hi].contiguous(),
                             [eps[0][b:b + 1, lo:hi].contiguous()])
            d = float((lpa[0] - lp[b, lo:hi]).abs().max())
            solo[(B, N, b, lo)] = d
            assert d <= 1e-5, (B, N, b, lo, d)
        # inverse(forward(x)) = x (the augmenter's inverse keeps the first input_dim dims of the latent)
        xr = h.inverse(z, ctx, extra, None)
        rel = float((xr - x).abs().max() / x.abs().max())
        print(f"B {B} N {N}: rows alone vs in the batch max {max(v for k, v in solo.items() if k[:2] == (B, N)):.1e}; round trip rel {rel:.2e}")
        assert rel < 1e-4


# ------------------------------------------------------------------------------------------------ full depth, native shape
def test_full_depth_native_shape_d2_150():
    """20 scenes x 1024 target points, 1250 context points, latent 300 (d2 = 150), 115 ExponentialCoupling layers: conditioned weights as
    fullsize_util.build_conditioned makes them, with each coupling's shift / reshift nudged (+-0.002 / +-0.0005, before the ActNorm statistics
    are taken) so that W is not a near-zero matrix; the whole batch finite, 32 rows of scene 0 against the fp64 oracle."""
    B, N, M, n = 20, 1024, 1250, 32
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", sample_size=N, flow_type="ExponentialCoupling")
    torch.manual_seed(11)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for t in md["flow"].modules():
            if type(t).__name__ == "ExponentialCoupling":
                t.shift.fill_(float(torch.rand(1, generator=g) * 0.004 - 0.002))
                t.reshift.fill_(float(torch.rand(1, generator=g) * 0.001 - 0.0005))
    c0, c1, cx, ce = synth_pairs(2, N, N, 999, cfg["latent_dim"] - cfg["input_dim"])
    condition_flow(md, cfg, (c0.to(DEV), c1.to(DEV), cx.to(DEV)), eps=[ce.to(DEV)])
    e0, e1, extra, eps = synth_pairs(B, M, N, 43)
    t0 = time.time()
    _, lp, _ = fa.inner_loop((e0.to(DEV), e1.to(DEV), extra.to(DEV)), md, cfg, eps=[eps.to(DEV)])
    torch.cuda.synchronize()
    print(f"native shape forward: {time.time() - t0:.2f} s")
    assert lp.shape == (B, N) and torch.isfinite(lp).all()
    ctx = md["input_embedder"](e0[:1].to(DEV)).cpu()
    c = dict(cfg)
    c["sample_size"] = n
    (lp64, margin), (lp32, _) = side_by_side(
        lambda: oracle_flow_rows(c, md, ctx, e1[:1, :n], extra[:1], [eps[:1, :n]], torch.float64),
        lambda: oracle_flow_rows(c, md, ctx, e1[:1, :n], extra[:1], [eps[:1, :n]], torch.float32))
    check_rows_against_fp64("native shape 20 x 1024 / 1250 x 115 ExponentialCoupling layers (d2 = 150), scene 0 rows 0..31",
                            lp[0, :n].cpu(), lp64, lp32, margin)
