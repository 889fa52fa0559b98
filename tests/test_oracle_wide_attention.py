"""The wide-attention fixtures (tests/golden/gen_golden_wide_attention.py: inner dims 256, 2 x 80 = 160 and 2 x 48 = 96, produced by running
the reference) pin the oracle side: the pure-torch oracle must reproduce their values, gradient records and attention weights within the
gates of test_oracle_golden.py / test_oracle_grads.py / test_oracle_attention_weights.py, whose bodies run here on these cases.  CPU only."""
import numpy as np
import pytest
import torch

import attn_weights_util as U
import test_oracle_golden as OG
import test_oracle_grads as OGR
from conftest import Fixture
from flowcompare_amd import train_ops as T

CASES = ["attn_i256", "attn_i160_heads", "attn_i96_cif"]
INNER = {"attn_i256": (1, 256), "attn_i160_heads": (2, 80), "attn_i96_cif": (2, 48)}


@pytest.mark.parametrize("case", CASES)
def test_fixture_configuration(case):
    fx = Fixture("e2e_" + case)
    heads, dim_head = INNER[case]
    assert (fx.cfg["cross_heads"], fx.cfg["cross_dim_head"]) == (heads, dim_head)
    assert (fx.meta["B"], fx.meta["N"], fx.meta["M"]) == (2, 20, 24)
    wq = [k for k in fx.sd_keys["flow"] if k.endswith(".attention.to_q.weight")]
    assert wq and all(fx.sd_keys["flow"][k][0] == heads * dim_head for k in wq)
    if case == "attn_i160_heads":
        assert fx.cfg["flow_type"] == "RationalQuadraticSplineCoupling" and fx.cfg["extra_z_value_context"] and "extra" in fx.a
    if case == "attn_i96_cif":
        assert fx.cfg["cif_latent_dim"] > fx.cfg["latent_dim"]


@pytest.mark.parametrize("case", CASES)
def test_oracle_fp64_reproduces_the_values(case):
    OG.test_forward_fp64_matches_reference("e2e_" + case)
    OG.test_per_transform_records_fp64("e2e_" + case)
    OG.test_inverse_fp64_matches_reference("e2e_" + case)
    OG.test_forward_fp32_close_to_reference_fp32("e2e_" + case)


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("case", CASES)
def test_oracle_autograd_reproduces_the_gradient_records(case, mode):
    OGR.test_oracle_autograd_matches_reference_backward(case, mode)


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_the_actnorm_init_records(case):
    OGR.test_oracle_actnorm_data_init_matches_reference(case)


@pytest.mark.parametrize("case", CASES)
def test_oracle_fp64_reproduces_the_attention_weights(case):
    """rtol = atol = 1e-9, as test_oracle_attention_weights.py."""
    fx, ref = Fixture("e2e_" + case), U.Weights("e2e_" + case)
    sd_flow, sd_emb = fx.state_dicts(torch.float64)
    batch = tuple(None if t is None else t.to(torch.float64) for t in (fx.t("extract_0"), fx.t("extract_1"), fx.t("extra")))
    rec, lp = U.oracle_weights(fx.derived_cfg(), sd_flow, sd_emb, batch, fx.eps(torch.float64))
    assert [p for p, _ in rec] == ref.prefixes and len(rec) == fx.cfg["n_flow_layers"] + 1
    np.testing.assert_allclose(lp.numpy(), fx.a["log_prob_f64"], rtol=1e-9, atol=1e-8)
    for i, (p, w) in enumerate(rec):
        assert tuple(w.shape) == (2, 20, 24) == ref.w64[i].shape and ref.w32[i].dtype == np.float32
        np.testing.assert_allclose(w.numpy(), ref.w64[i], rtol=1e-9, atol=1e-9)


def test_training_panel_widths_map_to_kernel_widths():
    """Every 32-padded panel width up to 256 runs on the next kernel width; above 256 is refused by name."""
    got = {d: T.AttentionFn._kernel_width(d) for d in range(32, 257, 32)}
    assert got == {32: 32, 64: 64, 96: 128, 128: 128, 160: 256, 192: 256, 224: 256, 256: 256}
    with pytest.raises(RuntimeError, match="256"):
        T.AttentionFn._kernel_width(288)
