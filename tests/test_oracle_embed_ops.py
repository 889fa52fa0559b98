"""Pins the fp64 references of the embedder training operators (tests/embed_ops_ref.py) to the oracle, and checks on the CPU that the
inputs committed for the GPU tests (tests/test_gpu_train_embed_ops.py) decide every arg-max and LeakyReLU branch by more than an fp32
kernel's error."""
import pytest
import torch

import embed_ops_ref as R
from oracle import flow_oracle as O
from oracle import paconv_oracle as PO

TOL = 1e-12


def _close(a, b):
    return R.rel(a, b) < TOL


def test_edge_bn_max_ref_equals_the_oracle_edge_conv_in_train_mode():
    g = torch.Generator().manual_seed(0)
    B, M, k, C, Co = 2, 40, 5, 6, 32
    f = torch.randn(B, M, C, generator=g, dtype=torch.float64)
    W = torch.randn(Co, 2 * C, generator=g, dtype=torch.float64) / (2 * C) ** 0.5
    gamma, beta = 0.5 + torch.rand(Co, generator=g, dtype=torch.float64), 0.3 * torch.randn(Co, generator=g, dtype=torch.float64)
    sd = {"conv1.0.weight": W.reshape(Co, 2 * C, 1, 1), "conv1.1.weight": gamma, "conv1.1.bias": beta}
    with O.train_mode():
        want = O.edge_conv(sd, 1, f, k)
    idx = (O.knn_indices(f, k) + (torch.arange(B) * M)[:, None, None]).reshape(B * M, k)
    f2 = f.reshape(B * M, C)
    wa, wb = W[:, :C], W[:, C:]
    out, mean, var, _ = R.edge_bn_max_ref(f2 @ wa.t(), f2 @ (wb - wa).t(), idx, gamma, beta, 0.2)
    assert _close(out.reshape(B, M, Co), want)
    e = torch.cat((f2[idx] - f2[:, None], f2[:, None].expand(-1, k, -1)), -1) @ W.t()
    assert _close(mean, e.mean((0, 1))) and _close(var, e.var((0, 1), unbiased=False))


def _paconv_sd(g, C, Cout, m):
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return {"L.scorenet.mlp_convs_hidden.0.weight": r(16, 3, 1, 1), "L.scorenet.mlp_bns_hidden.0.weight": 0.5 + r(16).abs(),
            "L.scorenet.mlp_bns_hidden.0.bias": 0.3 * r(16), "L.scorenet.mlp_convs_hidden.1.weight": r(m, 16, 1, 1) / 4,
            "L.scorenet.mlp_convs_hidden.1.bias": 0.3 * r(m), "L.weightbank": r(2 * C, m * Cout) / (2 * C) ** 0.5,
            "L.bn.weight": 0.5 + r(Cout).abs(), "L.bn.bias": 0.3 * r(Cout)}


def test_paconv_operator_references_compose_to_the_oracle_paconv_layer():
    g = torch.Generator().manual_seed(1)
    B, N1, K, C, Cout, m = 1, 6, 4, 5, 8, 8
    sd = _paconv_sd(g, C, Cout, m)
    in_feat = torch.randn(B, C, N1, K, generator=g, dtype=torch.float64)
    gxyz = torch.randn(B, 3, N1, K, generator=g, dtype=torch.float64)
    with O.train_mode():
        want = PO.paconv_layer(sd, "L", in_feat, gxyz, m).permute(0, 2, 3, 1).reshape(N1 * K, Cout)
    x = in_feat.permute(0, 2, 3, 1).reshape(N1 * K, C)
    gd = (gxyz - gxyz[..., :1]).permute(0, 2, 3, 1).reshape(N1 * K, 3)
    h = R.edge_bn_max_ref(gd @ sd["L.scorenet.mlp_convs_hidden.0.weight"][:, :, 0, 0].t(), None, None, sd["L.scorenet.mlp_bns_hidden.0.weight"],
                          sd["L.scorenet.mlp_bns_hidden.0.bias"], 0.0)[0]
    S = R.softmax_ref(h @ sd["L.scorenet.mlp_convs_hidden.1.weight"][:, :, 0, 0].t() + sd["L.scorenet.mlp_convs_hidden.1.bias"])
    G = R.centerdiff_ref(x, K) @ sd["L.weightbank"]
    o = R.assign_ref(S, G)
    assert _close(R.edge_bn_max_ref(o, None, None, sd["L.bn.weight"], sd["L.bn.bias"], 0.0)[0], want)
    # ... and the level's last layer: the max over each group of K consecutive rows (sa_module's x.max over the neighbours)
    ident = torch.arange(N1 * K).view(N1, K)
    assert _close(R.edge_bn_max_ref(o, None, ident, sd["L.bn.weight"], sd["L.bn.bias"], 0.0)[0], want.reshape(N1, K, Cout).max(dim=1)[0])


def test_group_ref_equals_the_oracle_grouping_and_kernel_input():
    g = torch.Generator().manual_seed(2)
    B, n, m, K, C = 2, 12, 3, 4, 5
    xyz = torch.randn(B, n, 3, generator=g, dtype=torch.float64)
    feat = torch.randn(B, C, n, generator=g, dtype=torch.float64)
    new_xyz = xyz[:, :m].contiguous()
    nidx = torch.randint(0, n, (B, m, K), generator=g)
    gx = PO.grouping(xyz.transpose(1, 2).contiguous(), nidx)
    x = torch.cat((gx - new_xyz.transpose(1, 2)[..., None], PO.grouping(feat, nidx)), 1)                  # sa_module
    want_E = torch.cat((x - x[..., :1], x), 1).permute(0, 2, 3, 1).reshape(B * m * K, -1)                  # paconv_layer's kernel input
    want_gd = (gx - gx[..., :1]).permute(0, 2, 3, 1).reshape(B * m * K, 3)
    E, gd = R.group_ref(feat.permute(0, 2, 1).reshape(B * n, C), xyz.reshape(B * n, 3), new_xyz.reshape(B * m, 3), nidx.reshape(B * m, K), B, n, m)
    assert _close(E, want_E) and _close(gd, want_gd)


def test_interp_ref_equals_the_oracle_interpolation():
    # paconv_oracle.interpolation is plain torch (it needs no compiled helper), so this case always runs
    g = torch.Generator().manual_seed(3)
    B, n, mk, C = 2, 9, 5, 7
    feat = torch.randn(B, C, mk, generator=g, dtype=torch.float64)
    idx = torch.randint(0, mk, (B, n, 3), generator=g)
    w = torch.rand(B, n, 3, generator=g, dtype=torch.float64)
    w = w / w.sum(-1, keepdim=True)
    want = PO.interpolation(feat, idx, w).permute(0, 2, 1).reshape(B * n, C)
    gidx = (idx + (torch.arange(B) * mk)[:, None, None]).reshape(B * n, 3)
    assert _close(R.interp_ref(feat.permute(0, 2, 1).reshape(B * mk, C), gidx, w.reshape(B * n, 3)), want)


@pytest.mark.parametrize("name", list(R.EDGE_CASES))
def test_committed_edge_inputs_are_decided(name):
    m = R.run_edge_ref(R.make_edge_case(name), torch.float64)["margins"]
    print(f"{name}: tau {m['tau']:.2e}  min gap {m['gap'].min().item():.2e}  min |u*| {m['ustar'].abs().min().item():.2e}")
    assert R.undecided(m) == 0


@pytest.mark.parametrize("name", list(R.POOL_CASES))
def test_committed_pool_inputs_are_decided(name):
    m = R.pool_margins(R.make_pool_case(name)[0].double())
    print(f"{name}: tau {m['tau']:.2e}  min gap {m['gap'].min().item():.2e}")
    assert R.undecided(m) == 0
