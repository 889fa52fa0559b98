"""The gate of tests/test_gpu_premlp.py must be able to fail (the precedent: tests/test_spline_edges_host.py).  On the CPU: the fp32
restatement of the pre-attention chain (tests/premlp_util.py restated32) passes max |q - q64| <= 16 e32 on every case of the GPU test's width
and activation sweeps; each of five planted faults -- small variants of the chain's arithmetic -- misses it on at least one case, and by a
stated margin: more than MARGIN = 6 times the HIGHEST gate the GPU test may ever take (64).  The fp64 reference itself is tied to
oracle.flow_oracle."""
import pytest
import torch

import premlp_util as PU
from oracle import flow_oracle as O

MAX_GATE, MARGIN = 64.0, 6.0
CASES = ([(k, "gelu", fam) for k in PU.WIDTHS for fam in PU.FAMILIES]
         + [(k, act, "plain") for k in (150, 90) for act in PU.ACT_NAMES if act != "gelu"])


def _ratio(c, fault=None):
    return c.ratio(PU.restated32(c.x, c.sd, c.act, fault))


def test_fp32_restatement_passes_the_gate_everywhere():
    worst = {}
    for k_in, act, fam in CASES:
        c = PU.case(k_in, 300, act, fam)
        r = _ratio(c)
        worst[fam] = max(worst.get(fam, 0.0), r)
        # the unit itself: |q| ~ 0.75, one fp32 ulp there is 6e-8; the worst of 19200 outputs behind five layers lies a few ulps out (here 2.8e-7 .. 6e-7)
        assert 1e-7 < c.e32 < 2e-6, f"{c.label()}: e32 {c.e32:.2e} is not an fp32 rounding error of a q of order 1"
        assert r <= PU.GATE, f"{c.label()}: the unfaulted restatement is at {r:.1f} e32"
    print("unfaulted fp32 restatement, worst |q - q64| / e32 per family:", {k: round(v, 2) for k, v in worst.items()})


@pytest.mark.parametrize("fault", PU.FAULTS)
def test_planted_fault_breaks_the_gate_with_margin(fault):
    """Measured on the CPU, |q - q64| / e32 as (smallest, largest) over the sweep's cases: fp16 activations 556 .. 983, variance over 255
    1890 .. 3394, tanh-GELU 368 .. 529, residual from hidden layer 0: 8e5 .. 1.3e6 -- each of these misses the gate at EVERY case.  eps 1e-6:
    5.0e4 .. 1.0e5 on `flat` and only 1.4 .. 13.4 on `plain`, inside the gate: that is why `flat` exists.  Asserted: the largest ratio is
    more than 6 x 64, and (all but eps) the smallest is above the gate of 16."""
    ratios = {}
    for k_in, act, fam in CASES:
        if fault == "tanh_gelu" and act != "gelu":
            continue
        ratios[(k_in, act, fam)] = _ratio(PU.case(k_in, 300, act, fam), fault)
    best = max(ratios, key=ratios.get)
    per_family = {fam: (min(r for (_, _, f), r in ratios.items() if f == fam), max(r for (_, _, f), r in ratios.items() if f == fam)) for fam in PU.FAMILIES}
    print(f"{fault}: |q - q64| / e32 (min, max) per family {({f: (round(a, 1), round(b, 1)) for f, (a, b) in per_family.items()})}, worst case {best}")
    assert ratios[best] > MARGIN * MAX_GATE, f"{fault} stays within {MARGIN} x the highest gate: {ratios[best]:.1f} e32 at {best}"
    if fault == "eps_1e-6":
        assert per_family["plain"][1] <= PU.GATE < per_family["flat"][0], "the flat family is what catches a wrong eps"
    else:
        assert min(ratios.values()) > PU.GATE, f"{fault} passes the gate at some case: {min(ratios.values()):.1f} e32"


def test_fp64_reference_is_the_oracle_chain():
    """premlp_util.chain in fp64 against oracle.flow_oracle on one model: O.mlp, then the query side of O.cross_attention, to 1e-12.  The
    oracle has no call that returns q, so its scores are read back through its own softmax: with I + 1 context points e_0 .. e_(I-1), 0 and
    identity K, V and `lin`, the attention output is w_j = softmax(q I^-0.5, 0)_j, and q_j I^-0.5 = log w_j - log(1 - sum w)."""
    c = PU.case(150, 300, "gelu", "plain")
    sd = {k: v.double() for k, v in c.sd.items()}
    h = O.mlp(sd, "net", c.x.double(), torch.nn.functional.gelu)
    I = sd["to_q.weight"].shape[0]
    eye = torch.eye(I, dtype=torch.float64)
    osd = {"a.norm.weight": sd["norm.weight"], "a.norm.bias": sd["norm.bias"], "a.fn.attention.to_q.weight": sd["to_q.weight"],
           "a.fn.attention.to_kv.weight": torch.cat((eye, eye), 0), "a.fn.lin.weight": eye, "a.fn.lin.bias": torch.zeros(I, dtype=torch.float64)}
    ctx = torch.cat((eye, torch.zeros(1, I, dtype=torch.float64)), 0)[None]      # [1, I + 1, I]: k_j = v_j = e_j, the last key and value 0
    w = O.cross_attention(osd, "a", h[None], ctx)[0]                             # [rows, I]
    q_oracle = (torch.log(w) - torch.log1p(-w.sum(-1, keepdim=True))) * PU.LOG2E
    assert (c.q64 - q_oracle).abs().max().item() < 1e-12
