"""Training path of ExponentialCoupling beyond d2 = 16: the forward (fc_train_expm_fwd_f32 dispatches d2 > 16 to the inference engine's
matrix-exponential action kernel) builds conditioned weights -- ActNorm's first-batch statistics -- at d2 = 150; the backward stays d2 <= 16
and refuses wider flows with a clear error before it launches anything."""
import pytest
import torch

import flowcompare_amd as fa
from flowcompare_amd import modules as M
from flowcompare_amd import train_ops as T
from flowcompare_amd.conditioning import condition_flow
from fullsize_util import synth_pairs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 256


@pytest.fixture(scope="module")
def wide():
    cfg = fa.named_config("c4_dgcnn_attn_extra_affine", sample_size=N, n_flow_layers=3, flow_type="ExponentialCoupling")
    torch.manual_seed(11)
    md = fa.initialize_flow(cfg, device=DEV, mode="test")
    c0, c1, cx, ce = synth_pairs(2, N, N, 999, cfg["latent_dim"] - cfg["input_dim"])
    condition_flow(md, cfg, (c0.to(DEV), c1.to(DEV), cx.to(DEV)), eps=[ce.to(DEV)])
    return cfg, md


def test_condition_flow_at_d2_150(wide):
    cfg, md = wide
    assert cfg["latent_dim"] - cfg["latent_dim"] // 2 == 150
    an = [m for m in md["flow"].modules() if isinstance(m, M.ActNormBijectionCloud)]
    assert an and all(float(m.initialized.item()) == 1.0 for m in an)
    assert all(torch.isfinite(m.log_scale).all() and torch.isfinite(m.shift).all() for m in an)
    e0, e1, extra, eps = synth_pairs(2, N, N, 5, cfg["latent_dim"] - cfg["input_dim"])
    md["flow"].eval()
    _, lp, bpd = fa.inner_loop((e0.to(DEV), e1.to(DEV), extra.to(DEV)), md, cfg, eps=[eps.to(DEV)])
    print(f"conditioned d2 = 150 flow: mean log p {float(lp.mean()):.3f}, bpd {float(bpd):.4f}")
    assert torch.isfinite(lp).all()


def test_training_backward_at_d2_150_raises_the_documented_error(wide):
    cfg, md = wide
    md["flow"].train()
    md["flow"].zero_grad()
    e0, e1, extra, eps = synth_pairs(2, N, N, 6, cfg["latent_dim"] - cfg["input_dim"])
    try:
        with pytest.raises(RuntimeError, match="ExponentialCoupling training backward supports d2 <= 16"):
            with T.step_guard(device=DEV):
                loss, _, _ = fa.inner_loop((e0.to(DEV), e1.to(DEV), extra.to(DEV)), md, cfg, eps=[eps.to(DEV)])
                assert torch.isfinite(loss)
                loss.backward()
    finally:
        md["flow"].eval()
