#!/usr/bin/env python3
"""Golden fixtures for cross-attention inner dimensions above 128 and for training above 64 (csrc/attention.hip attn_kernel<256>,
csrc/attention_weights.hip, csrc/train_attention.hip), produced by RUNNING THE REFERENCE through gen_golden.e2e_case (same synthesised
weights, same npz layout).  Every width except the attention's stays at gen_golden.TINY's values.

    python tests/golden/gen_golden_wide_attention.py

For each case it writes
  e2e_<case>.npz          forward / sampling fixture (gen_golden.e2e_case),
  attnw_e2e_<case>.npz    the reference's attn_weights of every attention, fp64 and fp32 run (recorder of gen_golden_attention_weights.py),
  grad_<case>.npz         eval / train / init gradient records (gen_golden_grads.grad_case).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import gen_golden as G  # noqa: E402
import gen_golden_attention_weights as AW  # noqa: E402
import gen_golden_grads as GG  # noqa: E402


def _case(name, cfg_name, over, **kw):
    orig_save = G.save

    def save_with_weights(n, cfg, arrays, meta=None):
        w, prefixes = AW._weight_arrays()
        AW._summary(n, w, prefixes)
        AW._write_weights(n, w)
        orig_save(n, cfg, arrays, meta)

    G.save = save_with_weights
    try:
        G.e2e_case(name, cfg_name, over, **kw)
    finally:
        G.save = orig_save


def main():
    torch.set_num_threads(8)
    sys.modules["models.perceiver"].F = AW._RecordingF()
    orig_run_forward = G.run_forward
    G.run_forward = AW._run_forward
    wide = dict(G.TINY)
    wide.update(cross_heads=1, cross_dim_head=256)
    _case("e2e_attn_i256", "swept-energy", dict(n_flow_layers=2, **wide), B=2, N=20, M=24, seed=61)
    # heads x dim_head = 2 x 80 = 160 (pads to 256: columns 160..255 are pad), spline coupling, extra context (dulcet-universe has it on)
    heads = dict(G.TINY)
    heads.update(cross_heads=2, cross_dim_head=80)
    _case("e2e_attn_i160_heads", "dulcet-universe", dict(n_flow_layers=2, flow_type="RationalQuadraticSplineCoupling", **heads),
          B=2, N=20, M=24, seed=62)
    cif = dict(G.TINY)
    cif.update(cif_latent_dim=16, net_cif_dist_hidden_dims=[16, 16], affine_cif_hidden=[16, 16, 16], cross_heads=2, cross_dim_head=48)
    # seed: the first one from 63 on at which the reference's own fp32 and fp64 log-probs agree within 1e-4 AND its own sampling pass stays
    # below |x| = 100.  With these random weights the CIF blocks are violently expansive for most seeds: at 63 the reference's sample
    # reaches 8.5e8, at 64 it stops on a zero scale in its own slicer, at 65 its two precisions disagree by 300 nats on one point.
    _case("e2e_attn_i96_cif", "swept-energy", dict(n_flow_layers=3, **cif), B=2, N=20, M=24, seed=74, z_scale=0.05)
    G.run_forward = orig_run_forward
    sys.modules["models.perceiver"].F = AW.torch_F
    for c in ("e2e_attn_i256", "e2e_attn_i160_heads", "e2e_attn_i96_cif"):
        GG.grad_case(c)


if __name__ == "__main__":
    main()
