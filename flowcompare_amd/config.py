"""Config handling for the flow engine.

Accepts the reference's wandb-style yaml (`key: {desc: ..., value: ...}`,
utils.py:373-377 `config_loader`) as well as flat `key: value` files, and fills
model keys that a file omits with the values every shipped reference config
uses.
"""
import os

import yaml

# Values common to all five shipped reference configs (config/*.yaml).
DEFAULTS = dict(
    input_dim=6, latent_dim=300, cif_latent_dim=300, n_flow_layers=115, sample_size=1024,
    n_samples_context=1250, n_neighbors=40, flow_type="AffineCoupling", affine_scale_fn="sigmoid",
    permuter_type="LinearLU", linear_lu_eps=1.0e-5, act_norm=True, cif_act_norm=True,
    hidden_dims=[512, 512, 512], hidden_dims_embedder_out=[512, 512, 512, 512, 512, 512],
    pre_attention_mlp_hidden_dims=[256, 256, 256], net_augmenter_dist_hidden_dims=[512, 512, 512],
    net_cif_dist_hidden_dims=[64, 64], affine_cif_hidden=[256, 256, 256],
    attn_dim=512, attn_input_dim=256, input_embedding_dim=64, cross_heads=1, cross_dim_head=64, attn_dropout=0.0,
    coupling_block_nonlinearity="GELU", augmenter_dist="ConditionalNormal", use_attn_augment=True,
    input_embedder="DGCNNembedder", extra_z_value_context=False, num_bins_spline=8,
    eps_expm=1.0e-8, coupling_expm_algo="torch", clamp_dist=10.0, data_parallel=False, amp=False,
    cif_dist="ConditionalNormal", load_checkpoint=False,
    # ExponentialCoupling training at 17 <= d2 <= 160 (csrc/expm_wide.hip); off: the backward refuses d2 > 16
    expm_wide_backward=False,
    # training loop (train.py:44-60, 112-120; values of the reference's shipped yaml files)
    optimizer_type="Adam", lr=1.0e-4, weight_decay=0.0, grad_clip_val=1.0, min_lr=1.0e-10, lr_factor=0.8, patience=2000, batch_size=20,
)

CONFIG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")


def config_loader(path, **overrides):
    """Load a yaml config into a flat dict (same contract as the reference's utils.config_loader)."""
    if not os.path.exists(path) and os.path.exists(os.path.join(CONFIG_DIR, path)):
        path = os.path.join(CONFIG_DIR, path)
    with open(path) as f:
        raw = yaml.safe_load(f)
    cfg = dict(DEFAULTS)
    for k, v in raw.items():
        cfg[k] = v["value"] if isinstance(v, dict) and "value" in v else v
    cfg.update(overrides)
    return cfg


def named_config(name, **overrides):
    """One of the benchmark configurations C1..C4, shipped under flowcompare_amd/configs/."""
    return config_loader(os.path.join(CONFIG_DIR, name + ".yaml"), **overrides)
