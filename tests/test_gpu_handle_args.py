"""Argument checks of the engine handles (flowcompare_amd/engine.py) that no other test reaches: every case is a host-side refusal
before the library is called, or one normal forward on a tiny fixture.  Error texts are pinned by their distinctive words."""
import functools

import pytest
import torch

import flowcompare_amd as fa
from conftest import Fixture
from flowcompare_amd import modules as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _case(name):
    """(handle, x, context, extra_context, eps, flow module, fixture) of one tiny fixture: built once, never modified."""
    fx = Fixture(name)
    cfg = dict(fx.cfg)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    sd_flow, sd_emb = fx.state_dicts()
    fa.load_flow({"flow": sd_flow, "input_embedder": sd_emb}, md)
    N = fx.meta["N"]
    ctx = fx.t("emb_f64").float().to(DEV)
    if ctx.dim() == 2:
        ctx = ctx[:, None, :].expand(-1, N, -1)
    extra = fx.t("extra")
    extra = None if extra is None else extra.to(DEV)[:, None, :].expand(-1, N, -1)
    return md["flow"]._engine(), fx.t("extract_1").to(DEV), ctx, extra, [e.to(DEV) for e in fx.eps()], md["flow"], fx


def test_log_prob_refuses_a_wrong_number_of_noise_tensors():
    h, x, ctx, extra, eps, _, _ = _case("e2e_tiny_identity_aug")
    assert h.n_noise == 0 and eps == []
    with pytest.raises(RuntimeError, match=r"flow needs 0 noise tensors, got 1"):
        h.log_prob(x, ctx, extra, [torch.zeros(2, 20, 6, device=DEV)])
    h, x, ctx, extra, eps, _, _ = _case("e2e_tiny_cif")
    assert h.n_noise == 4 and h.noise_width == [6, 4, 4, 4]
    with pytest.raises(RuntimeError, match=r"flow needs 4 noise tensors, got 3"):
        h.log_prob(x, ctx, extra, eps[:3])


def test_log_prob_refuses_a_noise_tensor_of_the_wrong_width():
    h, x, ctx, extra, eps, _, _ = _case("e2e_tiny_cif")
    with pytest.raises(RuntimeError, match=r"noise tensor has shape \(2, 20, 3\), expected \(2, 20, 4\)"):
        h.log_prob(x, ctx, extra, eps[:3] + [eps[3][:, :, :3]])


def test_missing_extra_context_is_refused_by_log_prob_and_inverse():
    h, x, ctx, extra, eps, _, fx = _case("e2e_tiny_global_extra")
    assert h.X == 1 and extra is not None
    with pytest.raises(RuntimeError, match=r"built with extra context \(extra_z_value_context\) but extra_context is None"):
        h.log_prob(x, ctx, None, eps)
    with pytest.raises(RuntimeError, match=r"built with extra context \(extra_z_value_context\) but extra_context is None"):
        h.inverse(fx.t("sample_z").float().to(DEV), ctx[:1], None, None)


def test_log_prob_refuses_a_3d_extra_context_with_another_point_count():
    h, x, ctx, extra, eps, _, _ = _case("e2e_tiny_global_extra")
    with pytest.raises(RuntimeError, match=r"Sizes of tensors must match: extra_context has 23 points, x has 24"):
        h.log_prob(x, ctx, extra[:, :23], eps)


def test_inverse_refuses_a_wrong_noise_count():
    h, x, ctx, extra, eps, _, fx = _case("e2e_tiny_cif")
    inv_eps = [e.to(DEV) for e in fx.eps(prefix="inveps")]
    assert len(inv_eps) == 3 and len(eps) == 4                       # one draw per CIF block backwards, the augmenter's on top forwards
    with pytest.raises(RuntimeError, match=r"inverse pass needs 3 noise tensors, got 4"):
        h.inverse(fx.t("sample_z").float().to(DEV), ctx[:1], None, eps)


def test_inverse_refuses_a_context_of_another_batch():
    h, x, ctx, extra, eps, _, fx = _case("e2e_tiny_identity_aug")
    with pytest.raises(RuntimeError, match=r"context batch 2 != latent batch 1"):
        h.inverse(fx.t("sample_z").float().to(DEV), ctx, None, None)


@pytest.mark.parametrize("entry", ["attention_weights", "attention_mass"])
def test_probe_entries_refuse_an_empty_layer_list(entry):
    h, x, ctx, extra, eps, _, _ = _case("e2e_tiny_cif")
    with pytest.raises(RuntimeError, match=entry + r": no layers requested"):
        getattr(h, entry)(x, ctx, extra, eps, [])


def test_handles_refuse_a_cpu_module():
    fx = Fixture("e2e_tiny_cif")
    md = fa.initialize_flow(dict(fx.cfg), device="cpu", mode="test")
    with pytest.raises(RuntimeError, match=r"the flow must be on a HIP device"):
        md["flow"]._engine()
    assert isinstance(md["input_embedder"], M.DGCNNembedder)
    with pytest.raises(RuntimeError, match=r"the embedder must be on a HIP device"):
        md["input_embedder"]._engine()
    with pytest.raises(RuntimeError, match=r"the embedder must be on a HIP device"):
        M.PointNet2SSGSeg(c=3, k=10, out_mlp_dims=(32, 32)).eval()._engine()


def test_the_three_forward_entries_are_one_pass():
    """log_prob, attention_weights and attention_mass run the same forward: with the same noise their log-probs are the same bytes."""
    h, x, ctx, extra, eps, flow, _ = _case("e2e_tiny_cif")
    ids = flow._probe_layer_ids(flow.attention_layers(), "test")
    assert ids == [-1, 0, 1, 2]
    lp = h.log_prob(x, ctx, extra, eps)
    w, lp_w = h.attention_weights(x, ctx, extra, eps, ids, return_log_prob=True)
    m, lp_m = h.attention_mass(x, ctx, extra, eps, ids, return_log_prob=True)
    assert torch.isfinite(lp).all()
    assert torch.equal(lp, lp_w) and torch.equal(lp, lp_m)
    assert [tuple(t.shape) for t in w] == [(2, 20, 24)] * 4 and [tuple(t.shape) for t in m] == [(2, 24)] * 4
