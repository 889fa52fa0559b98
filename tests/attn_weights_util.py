"""Shared by the attention-weight tests (CPU: test_oracle_attention_weights.py, GPU: test_gpu_attention_weights.py): the weight fixtures
written by tests/golden/gen_golden_attention_weights.py, and a recorder that pins the ORACLE's attention weights without editing
oracle/: it wraps oracle.flow_oracle.cross_attention (which _augment and _precondition look up by its module-level name) and
recomputes softmax(LN(h) Wq^T . (ctx Wk^T)^T . inner^-1/2) from the arguments of every call."""
import contextlib
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN, Fixture
from oracle import flow_oracle as O

# (weight file, fixture with the inputs).  The sharp case is a fixture of its own; the others reuse existing fixtures' inputs.
CASES = {"e2e_dulcet_L3": "e2e_dulcet_L3", "e2e_spline_L2": "e2e_spline_L2", "e2e_tiny_cif": "e2e_tiny_cif", "attnw_sharp_L3": "attnw_sharp_L3"}
SHARP = "attnw_sharp_L3"


class Weights:
    """attnw_<case>.npz: w64[i] / w32[i] = the reference's attn_weights [B, N, M] of attention i (call order) in its fp64 / fp32 run."""

    def __init__(self, case):
        z = np.load(os.path.join(GOLDEN, f"attnw_{case}.npz"))
        self.prefixes = json.loads(bytes(z["prefixes_json"]).decode())
        self.w64 = [z[f"w_f64_{i}"] for i in range(len(self.prefixes))]
        self.w32 = [z[f"w_f32_{i}"] for i in range(len(self.prefixes))]


def state_dicts(fx, dtype=torch.float32):
    """Fixture.state_dicts plus the to_q gain of the sharp fixture (meta_json), applied exactly as the generator applied it."""
    sd_flow, sd_emb = fx.state_dicts(dtype)
    gain = fx.meta.get("to_q_gain")
    if gain:
        for k in sd_flow:
            if k.endswith(".attention.to_q.weight"):
                sd_flow[k] = sd_flow[k] * gain
    return sd_flow, sd_emb


def layer_of(cfg, prefix):
    """state-dict prefix of an attention -> the `layers` entry of fa.attention_weights ("aug" or the 0-based flow-layer index)."""
    if prefix == "transforms.0.attn":
        return "aug"
    idx = int(prefix.split(".")[1])
    stride = 2 + (1 if cfg["act_norm"] else 0)
    assert prefix.endswith(".pre_conditioner.attn") and (idx - 1) % stride == 0
    return (idx - 1) // stride


@contextlib.contextmanager
def recording_oracle():
    """Inside the block every oracle.flow_oracle.cross_attention call appends (prefix, weights [B, N, M]) to the yielded list."""
    rec = []
    orig = O.cross_attention

    def wrapped(sd, prefix, h, ctx):
        wq = sd[f"{prefix}.fn.attention.to_q.weight"]
        wkv = sd[f"{prefix}.fn.attention.to_kv.weight"]
        inner = wq.shape[0]
        hn = F.layer_norm(h, (h.shape[-1],), sd[f"{prefix}.norm.weight"], sd[f"{prefix}.norm.bias"], 1e-5)
        q = hn @ wq.t()
        k = (ctx @ wkv.t())[..., :inner]
        rec.append((prefix, torch.softmax((q @ k.transpose(1, 2)) * (inner ** -0.5), dim=-1).detach()))
        return orig(sd, prefix, h, ctx)

    O.cross_attention = wrapped
    try:
        yield rec
    finally:
        O.cross_attention = orig


def oracle_weights(cfg, sd_flow, sd_emb, batch, eps, dtype=torch.float64):
    """oracle.inner_loop in `dtype` with the recorder on -> ([(prefix, w)], log_prob)."""
    cast = lambda t: None if t is None else t.to(dtype)
    sd_f = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd_flow.items()}
    sd_e = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd_emb.items()}
    with torch.no_grad(), recording_oracle() as rec:
        _, lp, _ = O.inner_loop(cfg, sd_f, sd_e, tuple(cast(t) for t in batch), [cast(e) for e in eps])
    return rec, lp


def gate(err_f32, wmax):
    """The 4 x E bound of the attention-weight tests: E = max(the fp32 yardstick's own distance from fp64, 4 * 2^-24 * largest weight)
    -- the floor is for rows where eager fp32 sits at its own rounding limit (a weight passes through four rounded steps here:
    exp2, the row sum, the reciprocal, the product); 4 = twice the 2x this project's HIP arithmetic has measured against eager fp32."""
    return 4.0 * max(float(err_f32), 4.0 * 2.0 ** -24 * float(wmax))


def load_case(case):
    return Fixture(CASES[case]), Weights(case)
