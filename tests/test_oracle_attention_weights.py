"""The attention-weight fixtures (tests/golden/attnw_*.npz: the reference's own `attn_weights`, models/perceiver.py:108-115) pin the
oracle side -- the fp64 oracle, through the recorder of attn_weights_util, must reproduce them -- and the host surface of the
feature (fa.attention_weights, ABI 9) exists.  No GPU needed."""
import numpy as np
import pytest
import torch

import attn_weights_util as U
import flowcompare_amd as fa
from flowcompare_amd import engine


def _batch(fx, dtype):
    return tuple(None if t is None else t.to(dtype) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))


@pytest.mark.parametrize("case", list(U.CASES))
def test_oracle_fp64_reproduces_the_reference_attention_weights(case):
    """rtol = atol = 1e-9: the bound test_oracle_golden.py uses for its fp64-vs-fp64 comparisons of latents and embeddings."""
    fx, ref = U.load_case(case)
    sd_flow, sd_emb = U.state_dicts(fx, torch.float64)
    rec, lp = U.oracle_weights(fx.derived_cfg(), sd_flow, sd_emb, _batch(fx, torch.float64), fx.eps(torch.float64))
    assert [p for p, _ in rec] == ref.prefixes
    np.testing.assert_allclose(lp.numpy(), fx.a["log_prob_f64"], rtol=1e-9, atol=1e-8)
    for i, (p, w) in enumerate(rec):
        assert tuple(w.shape) == (fx.meta["B"], fx.meta["N"], fx.meta["M"]) == ref.w64[i].shape
        print(f"{case} attention {i} {p}: max |oracle - reference| {np.abs(w.numpy() - ref.w64[i]).max():.1e}")
        np.testing.assert_allclose(w.numpy(), ref.w64[i], rtol=1e-9, atol=1e-9)


def test_sharp_fixture_is_sharp():
    """Condition on the fixture (not a tolerance): in every recorded attention the median over rows of the row maximum is >= 10 / M
    (the synthesised weights alone give ~ 1.02 / M; the fixture's to_q gain is in its meta_json)."""
    fx, ref = U.load_case(U.SHARP)
    M = fx.meta["M"]
    assert fx.meta["to_q_gain"] > 1 and len(ref.prefixes) == 4
    for i, w in enumerate(ref.w64):
        med = float(np.median(w.max(-1)))
        print(f"attention {i}: median row max {med * M:.1f}/M, reference fp32-vs-fp64 {np.abs(ref.w32[i] - w).max():.1e}")
        assert med >= 10.0 / M
        np.testing.assert_allclose(w.sum(-1), 1.0, rtol=0, atol=1e-12)
    assert np.isfinite(fx.a["log_prob_f64"]).all()


def test_layer_ids_of_the_fixture_prefixes():
    fx, ref = U.load_case("e2e_tiny_cif")
    assert [U.layer_of(fx.cfg, p) for p in ref.prefixes] == ["aug", 0, 1, 2]
    fx, ref = U.load_case("e2e_spline_L2")
    assert [U.layer_of(fx.cfg, p) for p in ref.prefixes] == ["aug", 0, 1]


def test_host_surface():
    assert callable(fa.attention_weights) and "attention_weights" in fa.__all__
    assert engine.ABI_VERSION == 10
    assert "fc_flow_attention_weights_f32" in engine.EXPORTS and "fc_op_attention_weights_f32" in engine.EXPORTS
    assert hasattr(engine.FlowHandle, "attention_weights") and callable(engine.op_attention_weights)


def test_cpu_model_raises_like_inner_loop():
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=1, sample_size=16)
    md = fa.initialize_flow(cfg, device="cpu", mode="test")
    batch = (torch.rand(1, 48, 6), torch.rand(1, 16, 6), torch.rand(1, 1))
    with pytest.raises(RuntimeError, match="HIP device|no CPU path"):
        fa.attention_weights(batch, md, cfg, layers=("aug", 0), points=[0, 1])
    with pytest.raises(RuntimeError, match="HIP device|no CPU path"):
        fa.inner_loop(batch, md, cfg)


def test_train_mode_and_bad_layers_raise_before_any_device_work():
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", n_flow_layers=2, sample_size=16)
    md = fa.initialize_flow(cfg, device="cpu", mode="test")
    x, ctx = torch.rand(1, 16, 6), torch.rand(1, 48, cfg["input_embedding_dim"])
    md["flow"].train()
    with pytest.raises(RuntimeError, match="eval-mode only"):
        md["flow"].attention_weights(x, context=ctx)
    md["flow"].eval()
    for bad in (2, -1, "layer0", 0.5):
        with pytest.raises(RuntimeError, match="out of range|unknown layer"):
            md["flow"].attention_weights(x, context=ctx, layers=(bad,))


def test_points_table_validation():
    dev = torch.device("cpu")
    with pytest.raises(RuntimeError, match="integer index tensor.*float32"):
        engine._points_table(torch.tensor([0.0, 1.0]), 2, 8, dev)
    with pytest.raises(RuntimeError, match=r"index 8 is not in \[0, 8\)"):
        engine._points_table(torch.tensor([0, 8]), 2, 8, dev)
    with pytest.raises(RuntimeError, match=r"index -1 is not in \[0, 8\)"):
        engine._points_table([[0, 1], [-1, 2]], 2, 8, dev)
    with pytest.raises(RuntimeError, match="shape"):
        engine._points_table(torch.zeros(3, 2, dtype=torch.long), 2, 8, dev)
    t, P, per = engine._points_table([[7, 0, 7], [1, 1, 2]], 2, 8, dev)
    assert t.dtype == torch.int32 and P == 3 and per == 1
    t, P, per = engine._points_table(torch.tensor([3, 1]), 2, 8, dev)
    assert P == 2 and per == 0
    assert engine._points_table(None, 2, 8, dev) == (None, 8, 0)
