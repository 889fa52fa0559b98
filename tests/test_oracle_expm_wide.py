"""Pins the CPU oracle (oracle/flow_oracle.py) at ExponentialCoupling widths beyond d2 = 16: the fixtures of
tests/golden/gen_golden_expm_wide.py, produced by running the reference (d2 = 20 'torch', d2 = 21 'original', d2 = 150 at real dims)."""
import numpy as np
import pytest
import torch

from conftest import Fixture
from oracle import flow_oracle as O

EXPWIDE = ["e2e_expwide_d20", "e2e_expwide_d21_orig", "e2e_expwide_L2"]


def _batch(fx, dtype):
    return fx.t("extract_0", dtype), fx.t("extract_1", dtype), fx.t("extra", dtype)


@pytest.mark.parametrize("name", EXPWIDE)
def test_oracle_forward_fp64_matches_reference_at_wide_d2(name):
    fx = Fixture(name)
    cfg = fx.derived_cfg()
    d2 = cfg["latent_dim"] - cfg["latent_dim"] // 2
    assert cfg["flow_type"] == "ExponentialCoupling" and d2 > 16
    sd_flow, sd_emb = fx.state_dicts(torch.float64)
    e0, e1, ex = _batch(fx, torch.float64)
    rec = []
    with torch.no_grad():
        loss, lp, bpd = O.inner_loop(cfg, sd_flow, sd_emb, (e0, e1, ex), fx.eps(torch.float64))
        emb = O.context_embed(cfg, sd_emb, e0)
        extra = None if ex is None else ex[:, None, :].expand(-1, e1.shape[1], -1)
        O.flow_log_prob(cfg, sd_flow, e1, emb, extra, fx.eps(torch.float64), record=rec)
    np.testing.assert_allclose(lp.numpy(), fx.a["log_prob_f64"], rtol=1e-9, atol=1e-8)
    assert abs(float(bpd) - float(fx.a["bpd_f64"])) < 1e-10
    ldj = torch.stack([torch.as_tensor(r[1]).expand(e1.shape[:2]) for r in rec]).numpy()
    np.testing.assert_allclose(ldj, fx.a["ldj_f64"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(rec[-1][0][:, :8].numpy(), fx.a["z_last_f64"], rtol=1e-9, atol=1e-9)
