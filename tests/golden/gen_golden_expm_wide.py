#!/usr/bin/env python3
"""Golden fixtures for ExponentialCoupling beyond d2 = 16 (the wide matrix-exponential action kernel, csrc/expm_wide.hip),
produced by RUNNING THE REFERENCE through gen_golden.e2e_case (same synthesised weights, same npz layout).

    python tests/golden/gen_golden_expm_wide.py     # writes tests/golden/e2e_expwide_*.npz

Prints the range of the coupling matrices' 1-norms ||W||_1 the reference exponentiated (forward and sampling passes alike).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import gen_golden as G  # noqa: E402

_NORMS = []


def _recording_expm(x, eps, algo="torch"):
    _NORMS.append(x.detach().abs().sum(dim=-2).amax(dim=-1).flatten().double())      # max column sum per matrix
    return G.ref_utils.expm(x, eps, algo=algo)


def _case(name, cfg_name, over, **kw):
    _NORMS.clear()
    G.e2e_case(name, cfg_name, over, **kw)
    n = torch.cat(_NORMS)
    print(f"   ||W||_1 over {n.numel()} matrices: min {n.min():.3f}  median {n.median():.3f}  max {n.max():.3f}")


def main():
    torch.set_num_threads(8)
    sys.modules["models.exponential_coupling"].expm = _recording_expm
    tiny = dict(G.TINY)
    tiny.update(latent_dim=40, cif_latent_dim=40)
    _case("e2e_expwide_d20", "swept-energy",
          dict(n_flow_layers=2, flow_type="ExponentialCoupling", coupling_expm_algo="torch", **tiny), B=2, N=20, M=24, seed=41)
    # latent 41 (d1 = 20, d2 = 21) is refused by the reference itself: its attention pre-conditioner splits x into two halves of
    # latent_dim // 2 (models/cif_block.py:15); latent 42 gives the same odd d2 = 21
    tiny.update(latent_dim=42, cif_latent_dim=42)
    _case("e2e_expwide_d21_orig", "swept-energy",
          dict(n_flow_layers=2, flow_type="ExponentialCoupling", coupling_expm_algo="original", **tiny), B=2, N=20, M=24, seed=42)
    _case("e2e_expwide_L2", "swept-energy", dict(n_flow_layers=2, flow_type="ExponentialCoupling"), B=1, N=32, M=48, seed=43)


if __name__ == "__main__":
    main()
