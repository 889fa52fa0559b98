"""The K|V fold of the inference engine (csrc/flow_pack.cpp build_attn), checked on the CPU in fp64 against the
oracle's cross attention (oracle/flow_oracle.py::cross_attention, reference models/perceiver.py:89-115):

    q k^T             = LN(h) (Wk^T Wq)^T ctx^T
    lin(softmax . v)  = (softmax . ctx) (Wlin Wv)^T + b

so that keys and values of every attention are the context embedding itself, and the gate that decides where the fold applies."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import flow_oracle as O

PREFIX = "transforms.1.pre_conditioner.attn"


def _weights(a_in, inner, E, attn_dim, seed):
    """seeded attention weights at the given widths, scaled like nn.Linear's default init (uniform in +-1/sqrt(fan_in))"""
    g = torch.Generator().manual_seed(seed)

    def u(*shape, fan_in):
        return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) / fan_in ** 0.5

    return {
        f"{PREFIX}.norm.weight": 1 + 0.1 * torch.randn(a_in, generator=g, dtype=torch.float64),
        f"{PREFIX}.norm.bias": 0.1 * torch.randn(a_in, generator=g, dtype=torch.float64),
        f"{PREFIX}.fn.attention.to_q.weight": u(inner, a_in, fan_in=a_in),
        f"{PREFIX}.fn.attention.to_kv.weight": u(2 * inner, E, fan_in=E),
        f"{PREFIX}.fn.lin.weight": u(attn_dim, inner, fan_in=inner),
        f"{PREFIX}.fn.lin.bias": u(attn_dim, fan_in=inner),
    }


def folded_cross_attention(sd, prefix, h, ctx):
    """What the engine computes once to_kv is folded away: the q projection ends in the context's columns (Wk^T Wq), the softmax weighs
    the context rows themselves, and lin starts from them (Wlin Wv).  The scale stays that of the inner width."""
    wq = sd[f"{prefix}.fn.attention.to_q.weight"]
    wkv = sd[f"{prefix}.fn.attention.to_kv.weight"]
    inner = wq.shape[0]
    wk, wv = wkv[:inner], wkv[inner:]
    wq_f = wk.t() @ wq                                               # [E, A_in]
    wlin_f = sd[f"{prefix}.fn.lin.weight"] @ wv                       # [attn_dim, E]
    hn = F.layer_norm(h, (h.shape[-1],), sd[f"{prefix}.norm.weight"], sd[f"{prefix}.norm.bias"], 1e-5)
    q = hn @ wq_f.t()
    w = torch.softmax((q @ ctx.transpose(1, 2)) * (inner ** -0.5), dim=-1)
    return F.linear(w @ ctx, wlin_f, sd[f"{prefix}.fn.lin.bias"])


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("ctx_scale", [1.0, 8.0])
def test_folded_attention_equals_the_oracle_in_fp64(seed, ctx_scale):
    """Real widths: LayerNorm over 256, q 256 -> 64, context embedding 64, lin 64 -> 512; 300 queries over 280 context points.  fp64 on both
    sides, so what is left is the reassociation of three matrix products: bounded by 1e-12 of the output's magnitude (the condition of a
    softmax over scores of order 1-10 times 2^-53 leaves four orders of magnitude of room)."""
    sd = _weights(256, 64, 64, 512, seed)
    g = torch.Generator().manual_seed(100 + seed)
    h = torch.randn(2, 300, 256, generator=g, dtype=torch.float64) * 3 + 0.5
    ctx = torch.randn(2, 280, 64, generator=g, dtype=torch.float64) * ctx_scale
    ref = O.cross_attention(sd, PREFIX, h, ctx)
    got = folded_cross_attention(sd, PREFIX, h, ctx)
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    print(f"seed {seed}, context scale {ctx_scale}: max |folded - oracle| / max |oracle| = {err:.2e}")
    assert ref.shape == (2, 300, 512) and err < 1e-12


def test_fold_needs_no_shape_change_only_at_equal_widths():
    """The folded q projection is [E, A_in] and the folded lin [attn_dim, E]: the packed shapes [inner, A_in] / [attn_dim, inner] are kept
    exactly when E == inner."""
    for E in (32, 64, 128):
        sd = _weights(256, 64, E, 512, 5)
        wkv = sd[f"{PREFIX}.fn.attention.to_kv.weight"]
        wq_f = wkv[:64].t() @ sd[f"{PREFIX}.fn.attention.to_q.weight"]
        wlin_f = sd[f"{PREFIX}.fn.lin.weight"] @ wkv[64:]
        assert (wq_f.shape == sd[f"{PREFIX}.fn.attention.to_q.weight"].shape) == (E == 64)
        assert (wlin_f.shape == sd[f"{PREFIX}.fn.lin.weight"].shape) == (E == 64)


def test_gate_refuses_other_widths_and_biased_projections():
    """The engine's gate (csrc/flow_pack.cpp kv_fold_gate_dims, host code; read through fc_debug_kv_fold_gate without a device): the fold is
    taken when the embedding is as wide as the attention's inner dimension, the two pad to the same kernel width (the embedding panel to a
    multiple of 32, the inner dimension to 32 / 64 / 128: 65..96 do not) and neither to_q nor to_kv has a bias, and only then."""
    from flowcompare_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        pytest.fail(f"{engine.LIB_PATH} not built")
    lib = ctypes.CDLL(engine.LIB_PATH)
    gate = lib.fc_debug_kv_fold_gate
    gate.restype = ctypes.c_int32
    for E in (8, 32, 33, 64, 97, 128):
        assert gate(E, E, 0, 0) == 1, E
    for E, inner in ((32, 64), (128, 64), (64, 32), (60, 64), (0, 0), (65, 65), (80, 80), (96, 96), (129, 129), (160, 160)):
        assert gate(E, inner, 0, 0) == 0, (E, inner)
    assert gate(64, 64, 1, 0) == 0 and gate(64, 64, 0, 1) == 0 and gate(64, 64, 1, 1) == 0
    # with a bias on to_kv the algebra indeed fails: k = Wk ctx + bk adds a per-query constant to the scores (harmless under the softmax) but
    # v = Wv ctx + bv adds Wlin bv to the output, and a bias on to_q adds bq . (Wk ctx) per key -- terms the folded weights have no place for
    sd = _weights(256, 64, 64, 512, 7)
    g = torch.Generator().manual_seed(8)
    h = torch.randn(1, 40, 256, generator=g, dtype=torch.float64)
    ctx = torch.randn(1, 50, 64, generator=g, dtype=torch.float64)
    bq = torch.randn(64, generator=g, dtype=torch.float64)
    wq, wkv = sd[f"{PREFIX}.fn.attention.to_q.weight"], sd[f"{PREFIX}.fn.attention.to_kv.weight"]
    hn = F.layer_norm(h, (256,), sd[f"{PREFIX}.norm.weight"], sd[f"{PREFIX}.norm.bias"], 1e-5)
    k, v = ctx @ wkv[:64].t(), ctx @ wkv[64:].t()
    biased = F.linear(torch.softmax(((hn @ wq.t() + bq) @ k.transpose(1, 2)) * 64 ** -0.5, -1) @ v, sd[f"{PREFIX}.fn.lin.weight"], sd[f"{PREFIX}.fn.lin.bias"])
    assert (biased - folded_cross_attention(sd, PREFIX, h, ctx)).abs().max().item() > 1e-3
