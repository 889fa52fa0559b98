"""Cross-attention inner dimensions up to 256 (attn_kernel<256>, attn_weights_kernel<256, 0>, the attention backward at head dims 128 and
256) in inference and training.  Operators against fp64 with the ratio convention of DESIGN.md section 11b (4 x E, E = the larger of eager
fp32's own distance from fp64 and 4 * 2^-24 of the tensor's scale); the engine and the training path against the reference fixtures of
tests/golden/gen_golden_wide_attention.py with the gates of test_gpu_flow.py, test_gpu_attention_weights.py and test_gpu_expm_wide_bwd.py.

Shapes: two scenes (scene strides); query counts that fill neither a 128-query workgroup nor a 32-query wave; one key, one key short of a
tile boundary (the 256-wide forward stages 32 keys, the weights kernel 64, the backward 32), a few tiles with a ragged tail."""
import math

import numpy as np
import pytest
import torch

import attn_weights_util as U
import flowcompare_amd as fa
from conftest import Fixture
from flowcompare_amd import engine
from flowcompare_amd import train_ops as T
from fullsize_util import build_conditioned, state_dicts, synth_pairs
from oracle import flow_oracle as O
from test_gpu_attention_weights import _against_oracle, _kernels, _ratio
from test_gpu_train import _rel, _train_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BPD_TOL, PER_POINT_TOL, MEAN_ABS_TOL = 1e-4, 2e-3, 3e-4          # tests/test_gpu_flow.py
FLOOR = 4.0 * 2.0 ** -24
OP_SHAPES = [(2, 150, 70), (1, 1, 1), (2, 33, 257), (1, 130, 1000)]
CASES = ["e2e_attn_i256", "e2e_attn_i160_heads", "e2e_attn_i96_cif"]
HEAD_DIM = {"e2e_attn_i256": 256, "e2e_attn_i160_heads": 256, "e2e_attn_i96_cif": 128}


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------ 1. operator, forward
@pytest.mark.parametrize("B,N,M", OP_SHAPES)
def test_operator_forward_at_256_matches_fp64(B, N, M):
    D = 256
    q, k, v = _rand(B, N, D, seed=1, scale=2.0), _rand(B, M, D, seed=2, scale=2.0), _rand(B, M, D, seed=3)     # as test_attention_matches_fp64
    scale = D ** -0.5
    y64 = torch.softmax(q.double() @ k.double().transpose(1, 2) * scale, -1) @ v.double()
    y32 = (torch.softmax(q @ k.transpose(1, 2) * scale, -1) @ v).double()
    with _kernels() as kn:
        y = engine.op_attention(q.to(DEV), k.to(DEV), v.to(DEV), scale).cpu()
    assert kn.ran("attn_kernel<256>"), kn.names
    assert y.shape == y64.shape and torch.isfinite(y).all()
    err, e32 = (y.double() - y64).abs().max().item(), (y32 - y64).abs().max().item()
    E = max(e32, FLOOR * y64.abs().max().item())
    print(f"op_attention D 256 B {B} N {N} M {M}: max |y - fp64| {err:.2e}   fp32 yardstick {e32:.2e}   ratio to E {err / E:.2f}  (gate 4)")
    assert err <= 4.0 * E


# ------------------------------------------------------------------ 2. operator, weights
@pytest.mark.parametrize("B,N,M", OP_SHAPES)
def test_operator_weights_at_256_match_fp64(B, N, M):
    D = 256
    q, k = _rand(B, N, D, seed=1, scale=2.0), _rand(B, M, D, seed=2, scale=2.0)
    sm = D ** -0.5
    w64 = torch.softmax(q.double() @ k.double().transpose(1, 2) * sm, -1)
    w32 = torch.softmax(q @ k.transpose(1, 2) * sm, -1)
    with _kernels() as kn:
        w = engine.op_attention_weights(q.to(DEV), k.to(DEV), sm)
    assert kn.ran("attn_weights_kernel<256, 0>"), kn.names
    assert tuple(w.shape) == (B, N, M) and w.dtype == torch.float32 and torch.isfinite(w).all() and (w >= 0).all()
    assert (w.double().sum(-1) - 1.0).abs().max().item() <= M * 2.0 ** -23
    err, bound = _ratio(f"op_attention_weights D 256 B {B} N {N} M {M}", w, w64, w32)
    assert err <= bound
    per = torch.randint(0, N, (B, 3), generator=torch.Generator().manual_seed(N + M))      # 3 points per scene
    got = engine.op_attention_weights(q.to(DEV), k.to(DEV), sm, points=per)
    assert tuple(got.shape) == (B, 3, M) and torch.equal(got, torch.stack([w[b, per[b]] for b in range(B)]))
    err, bound = _ratio("   the selected rows", got, torch.stack([w64[b, per[b]] for b in range(B)]), torch.stack([w32[b, per[b]] for b in range(B)]))
    assert err <= bound


def test_operators_name_the_widths_they_take():
    q, k = _rand(1, 4, 48, seed=1), _rand(1, 4, 48, seed=2)
    with pytest.raises(RuntimeError, match="D must be 32, 64 or 128, or 256"):
        engine.op_attention_weights(q.to(DEV), k.to(DEV), 1.0)
    with pytest.raises(RuntimeError, match="D must be 32, 64 or 128, or 256"):
        engine.op_attention(q.to(DEV), k.to(DEV), k.to(DEV), 1.0)


# ------------------------------------------------------------------ 3. operator, training
def _train_attention(q, k, v, dout, B, N, M, I, scale, fp16):
    """T.attention on leaf PANELS (so that the pad columns of the gradients are visible) -> (out, dq, dk, dv) panels."""
    qp, kp, vp = (T.to_panel(t.float().reshape(-1, I)).to(DEV).requires_grad_(True) for t in (q, k, v))
    with T.step_guard(fp16=fp16, device=DEV) as guard:
        op = T.attention(qp, kp, vp, B, N, M, scale)
        op.backward(T.to_panel(dout.float().reshape(-1, I)).to(DEV))
        assert not guard.overflowed()
    return op.detach(), qp.grad, kp.grad, vp.grad


@pytest.mark.parametrize("fp16", [True, False])
@pytest.mark.parametrize("B,N,M", [(2, 300, 77), (2, 50, 40), (1, 1, 1)])
@pytest.mark.parametrize("I", [96, 128, 129, 160, 256])
def test_training_attention_forward_and_backward_match_fp64(I, B, N, M, fp16):
    """The body of test_gpu_train.py::test_attention_forward_and_backward_match_fp64 (same draw, same _rel floors) at the wide inner
    dims, each tensor gated at 4 x the error of the identical computation in eager fp32 on the CPU (floor 4 * 2^-24 of its scale)."""
    g = torch.Generator().manual_seed(B * N + M)
    q, k, v = (torch.randn(B, n, I, generator=g).double() for n in (N, M, M))
    dout = torch.randn(B, N, I, generator=g).double()
    scale = I ** -0.5

    def eager(dtype):
        qq, kk, vv = (t.detach().clone().to(dtype).requires_grad_(True) for t in (q, k, v))
        o = torch.softmax(qq @ kk.transpose(1, 2) * scale, -1) @ vv
        o.backward(dout.to(dtype))
        return dict(out=o.detach().double(), dq=qq.grad.double(), dk=kk.grad.double(), dv=vv.grad.double())
    r64, r32 = eager(torch.float64), eager(torch.float32)
    panels = _train_attention(q, k, v, dout, B, N, M, I, scale, fp16)
    rows = dict(out=B * N, dq=B * N, dk=B * M, dv=B * M)
    floors = dict(out=1e-2, dq=1.0, dk=1.0, dv=1e-2)
    line = []
    for (name, p) in zip(("out", "dq", "dk", "dv"), panels):
        assert p.shape[1] == (I + 31) // 32 * 32 and torch.isfinite(p).all()
        assert not p[:, I:].any() and not p[rows[name]:].any(), f"{name}: pad columns / rows are not exactly zero"
        got = T.from_panel(p, rows[name], I).reshape(r64[name].shape)
        err, e32 = _rel(got, r64[name], floors[name]), _rel(r32[name], r64[name], floors[name])
        line.append(f"{name} {err:.1e} (fp32 {e32:.1e}, ratio {err / max(e32, FLOOR):.2f})")
        assert err <= 4.0 * max(e32, FLOOR), (name, err, e32)
    print(f"attention I {I} B {B} N {N} M {M} fp16 {fp16}: " + "  ".join(line))
    again = _train_attention(q, k, v, dout, B, N, M, I, scale, fp16)
    for a, b in zip(panels, again):
        assert torch.equal(a, b), "two runs differ"
    if B == 2:                                                       # the second scene alone: same bits as inside the launch of two
        solo = _train_attention(q[1:], k[1:], v[1:], dout[1:], 1, N, M, I, scale, fp16)
        for name, a, b in zip(("out", "dq", "dk", "dv"), panels, solo):
            n = rows[name] // 2
            assert torch.equal(a[n:2 * n], b[:n]), f"{name} of scene 1 depends on scene 0"


# ------------------------------------------------------------------ 4. engine against the reference
def _build(fx):
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    sd_flow, sd_emb = fx.state_dicts()
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    return cfg, md


@pytest.mark.parametrize("name", CASES)
def test_inner_loop_matches_reference_golden(name):
    fx = Fixture(name)
    cfg, md = _build(fx)
    batch = tuple(None if t is None else t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
    eps = [e.to(DEV) for e in fx.eps()]
    with _kernels() as kn:
        loss, lp, bpd = fa.inner_loop(batch, md, cfg, eps=eps)
    assert kn.ran(f"attn_kernel<{HEAD_DIM[name]}>"), kn.names
    lp = lp.cpu().double().numpy()
    d64 = np.abs(lp - fx.a["log_prob_f64"])
    print(f"{name}: vs fp64 golden max {d64.max():.2e} mean {d64.mean():.2e}; ref fp32 vs fp64 max "
          f"{np.abs(fx.a['log_prob_f32'] - fx.a['log_prob_f64']).max():.2e}; bpd diff {abs(float(bpd) - float(fx.a['bpd_f64'])):.2e}")
    assert np.isfinite(lp).all()
    assert abs(float(bpd) - float(fx.a["bpd_f64"])) < BPD_TOL
    assert d64.max() < PER_POINT_TOL and d64.mean() < MEAN_ABS_TOL


@pytest.mark.parametrize("name", CASES)
def test_make_sample_matches_reference_golden(name):
    """As tests/test_gpu_flow.py::test_make_sample_matches_reference_golden."""
    fx = Fixture(name)
    cfg, md = _build(fx)

    class FixedZ:
        def sample(self, num_samples, n_points=None, context=None):
            return fx.t("sample_z").float().to(DEV)

    md["flow"]._inverse_eps = [e.to(DEV) for e in fx.eps(prefix="inveps")] or None
    extra = fx.t("extra")
    x = fa.make_sample(24, fx.t("extract_0")[:1].to(DEV), md, cfg, sample_distrib=FixedZ(), extra_context=None if extra is None else extra[:1].to(DEV))
    d = np.abs(x.cpu().double().numpy() - fx.a["sample_x_f64"])
    scale = max(1.0, float(np.abs(fx.a["sample_x_f64"]).max()))
    print(f"{name}: sample max err {d.max():.2e} (|x|max {scale:.1f})")
    assert d.max() < 5e-4 * scale


@pytest.mark.parametrize("name", CASES)
def test_engine_matches_reference_weights(name):
    """Every attention of the fixture against the reference's fp64 rows, ratio <= 4 with the reference's fp32 run as the yardstick."""
    fx, ref = Fixture(name), U.Weights(name)
    cfg, md = _build(fx)
    batch = tuple(None if t is None else t.to(DEV) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
    layers = [U.layer_of(cfg, p) for p in ref.prefixes]
    assert layers == ["aug"] + list(range(cfg["n_flow_layers"]))
    with _kernels() as kn:
        ws, lp = fa.attention_weights(batch, md, cfg, layers=layers, eps=[e.to(DEV) for e in fx.eps()], return_log_prob=True)
    assert kn.ran(f"attn_weights_kernel<{HEAD_DIM[name]}, 0>"), kn.names
    assert torch.equal(lp, fa.inner_loop(batch, md, cfg, eps=[e.to(DEV) for e in fx.eps()])[1])
    for i, w in enumerate(ws):
        assert tuple(w.shape) == ref.w64[i].shape and w.dtype == torch.float32
        assert (w.double().sum(-1) - 1.0).abs().max().item() <= fx.meta["M"] * 2.0 ** -23
        err, bound = _ratio(f"{name} attention {i} ({layers[i]})", w, ref.w64[i], ref.w32[i])
        assert err <= bound


@pytest.mark.parametrize("name", CASES)
def test_log_prob_inverse_round_trip(name):
    """x -> latent (Flow.log_prob) -> Flow.inverse at the fixture size.  Without CIF blocks the inverse returns x: the augmented dims ride in
    the latent.  Bound: both passes are gated at 5e-4 of the sample's scale against fp64 (test_make_sample_matches_reference_golden), and the
    round trip of exact arithmetic is the identity.  A CIF block's inverse redraws the dims its slicer dropped, so no round trip exists
    there; and with the fixture's random weights that inverse is so expansive that unit noise overflows fp32 (the reference's own sampling
    pass runs from a latent scaled by 0.05, tests/golden/gen_golden_wide_attention.py).  There the forward's latent must be finite and the
    inverse, from the fixture's own sampling latent and noise, must return the same finite bits twice."""
    fx = Fixture(name)
    cfg, md = _build(fx)
    h = md["flow"]._engine()
    e0, x = fx.t("extract_0").to(DEV), fx.t("extract_1").to(DEV)[:, :, :cfg["input_dim"]].contiguous()
    ctx = md["input_embedder"](e0[:, :, :cfg["input_dim"]])
    extra = None if fx.t("extra") is None else fx.t("extra").to(DEV)
    lp, z = h.log_prob(x, ctx, extra, [e.to(DEV) for e in fx.eps()], return_latent=True)
    assert torch.isfinite(z).all()
    if cfg["cif_latent_dim"] > cfg["latent_dim"]:
        zs, inv_eps = fx.t("sample_z").float().to(DEV), [e.float().to(DEV) for e in fx.eps(prefix="inveps")]
        assert len(inv_eps) == cfg["n_flow_layers"]
        back = h.inverse(zs, ctx[:1], None if extra is None else extra[:1], inv_eps)
        assert tuple(back.shape) == (1, zs.shape[1], cfg["input_dim"]) and torch.isfinite(back).all()
        assert torch.equal(back, h.inverse(zs, ctx[:1], None if extra is None else extra[:1], inv_eps))
    else:
        back = h.inverse(z, ctx, extra, [])
        assert back.shape == x.shape and torch.isfinite(back).all()
        assert torch.equal(back, h.inverse(z, ctx, extra, []))
        err = (back - x).abs().max().item()
        print(f"{name}: round trip max |x' - x| {err:.2e}")
        assert err < 5e-4 * max(1.0, x.abs().max().item())


# ------------------------------------------------------------------ 5. training against the reference
@pytest.mark.parametrize("name", CASES)
def test_flow_backward_matches_oracle_autograd(name):
    """Procedure and gates of tests/test_gpu_expm_wide_bwd.py::test_flow_backward_at_wide_d2_matches_oracle_autograd."""
    fx = Fixture(name)
    cfg, md = _build(fx)
    loss, lp, x, ctx = _train_step(fx, cfg, md)
    c = fx.derived_cfg()
    sd_f, _ = fx.state_dicts(torch.float64)
    for v in sd_f.values():
        if v.is_floating_point():
            v.requires_grad_(True)
    e1 = fx.t("extract_1", torch.float64)[:, :, :c["input_dim"]].requires_grad_(True)
    ex = fx.t("extra", torch.float64)
    ex = None if ex is None else ex[:, None, :].expand(-1, e1.shape[1], -1)
    lp_o = O.flow_log_prob(c, sd_f, e1, ctx.detach().cpu().double(), ex, fx.eps(torch.float64))
    (-lp_o.mean()).backward()
    gn = sum(float((v.grad ** 2).sum()) for v in sd_f.values() if v.is_floating_point() and v.grad is not None) ** 0.5
    worst, worst_name, n_attn = 0.0, "", 0
    for n, p in md["flow"].named_parameters():
        if sd_f[n].grad is None:
            continue
        assert p.grad is not None, n
        n_attn += ".attention." in n
        e = (p.grad.double().cpu() - sd_f[n].grad).abs().sum().item() / max(sd_f[n].grad.abs().sum().item(), 1e-4 * gn)
        if e > worst:
            worst, worst_name = e, n
    assert n_attn >= 2 * (cfg["n_flow_layers"] + 1)
    print(f"{name}: loss diff {abs(loss.item() + lp_o.mean().item()):.1e} dx {_rel(x.grad, e1.grad):.1e}; worst parameter gradient L1 error {worst:.1e} ({worst_name})")
    assert abs(loss.item() + lp_o.mean().item()) < 2e-4 * max(1.0, abs(lp_o.mean().item())) and _rel(x.grad, e1.grad) < 5e-4 and worst < 1e-3


# ------------------------------------------------------------------ 6. real widths once
def test_real_widths_at_inner_256_against_the_oracle():
    """C4 with cross_dim_head = 256 (every other width as shipped), conditioned weights, on the HIP embedder's own context: the three
    golden gates against the fp64 oracle, and the weights of every attention as test_other_head_dims_against_the_oracle checks 96."""
    B, N, M = 2, 150, 333
    cfg, md = build_conditioned("c4_dgcnn_attn_extra_affine", N, DEV, n_flow_layers=2, cross_heads=1, cross_dim_head=256)
    e0, e1, extra, eps = synth_pairs(B, M, N, 6, cfg["latent_dim"] - cfg["input_dim"])
    emb = md["input_embedder"](e0.to(DEV)[:, :, :cfg["input_dim"]])
    ex_dev = extra.to(DEV)[:, None, :].expand(-1, N, -1)
    with _kernels() as kn:
        lp = md["flow"].log_prob(e1.to(DEV), context=emb, extra_context=ex_dev, eps=[eps.to(DEV)]).cpu().double()
    assert kn.ran("attn_kernel<256>"), kn.names
    sd_f, _ = state_dicts(md, torch.float64)
    with torch.no_grad():
        lp64 = O.flow_log_prob(cfg, sd_f, e1.double(), emb.cpu().double(), extra.double()[:, None, :].expand(-1, N, -1), [eps.double()])
    d = (lp - lp64).abs()
    bpd_gap = abs(float(lp.mean() - lp64.mean())) * math.log2(math.e) / cfg["input_dim"]
    print(f"C4 at inner 256: |log p - fp64| max {d.max():.2e} mean {d.mean():.2e}  bpd gap {bpd_gap:.2e}")
    assert torch.isfinite(lp).all() and d.max() < PER_POINT_TOL and d.mean() < MEAN_ABS_TOL and bpd_gap < BPD_TOL
    with _kernels() as kn:
        worst, ws = _against_oracle("inner dim 256", cfg, md, e0, e1, extra, [eps], ["aug", 0, 1])
    assert worst <= 1.0 and tuple(ws[0].shape) == (B, N, M) and kn.ran("attn_weights_kernel<256, 0>"), kn.names


def test_inner_257_is_refused_at_create():
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=1, sample_size=16, cross_heads=1, cross_dim_head=257)
    with pytest.raises(RuntimeError, match="256"):
        md = fa.initialize_flow(cfg, device=DEV, mode="test")
        md["flow"]._engine()
