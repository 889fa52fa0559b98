"""The pre-attention chain x1 -> in_layer -> two hidden layers -> out_layer -> LayerNorm -> q projection (models/cif_block.py:14-20,
models/perceiver.py:18-35, 104-106) on the host, for tests/test_gpu_premlp.py and tests/test_premlp_host.py: the fp64 reference, the same
chain in plain fp32 torch (its error against fp64, e32, is the unit of the gate), an fp32 restatement that can carry planted faults, and the
seeded case builder.

Gate:  max |q - q64| <= GATE * e32.  GATE = 16: the kernel's activations travel as two fp16 limbs, 22 significand bits against fp32's 24 --
four times coarser rounding per layer -- and another factor of four covers the summation order and the spread of a maximum over ~2 * 10^4
outputs.  Neither factor is taken from the kernel's measured error."""
import functools
import math

import torch
import torch.nn.functional as F

GATE = 16.0
LOG2E = 1.4426950408889634
ACT_NAMES = ("none", "gelu", "relu", "elu", "lrelu")                      # engine.OP_ACTS
ACTS = {"none": lambda t: t, "gelu": F.gelu, "relu": F.relu, "elu": F.elu, "lrelu": lambda t: F.leaky_relu(t, 0.2)}
FAULTS = ("fp16_acts", "eps_1e-6", "var_over_255", "tanh_gelu", "residual_from_hidden0")
MIN_ROW_STD = 0.005                                                       # every case: the row's standard deviation in front of LayerNorm (fp64)


def make_state(k_in, seed, inner=64, hidden=256, n_mid=2, family="plain", lu_dim=0):
    """Seeded uniform weights, scaled as tests/test_gpu_ops.py::_mlp_state: sqrt(3 / K), times 1.5 for the hidden layers, biases +-0.2,
    gamma = 1 +- 0.3, beta +- 0.2.  family "flat": out_layer's weight and bias times 0.01, so that a row's standard deviation in front of
    LayerNorm is about 0.01 and eps = 1e-5 is ~5 % of its variance (on "plain" a wrong eps stays inside the gate).  lu_dim = D > 0 adds
    the affine map of a pre-layer, lu.weight [D, D] and lu.bias [D]."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *sh, sc=1.0: (torch.rand(*sh, generator=g) * 2 - 1) * sc
    sd = {"net.in_layer.weight": u(hidden, k_in, sc=(3.0 / k_in) ** 0.5), "net.in_layer.bias": u(hidden, sc=0.2)}
    for i in range(n_mid):
        sd[f"net.layers.{i}.weight"] = u(hidden, hidden, sc=(3.0 / hidden) ** 0.5 * 1.5)
        sd[f"net.layers.{i}.bias"] = u(hidden, sc=0.2)
    flat = 0.01 if family == "flat" else 1.0
    assert family in ("plain", "flat")
    sd["net.out_layer.weight"] = u(256, hidden, sc=(3.0 / hidden) ** 0.5) * flat
    sd["net.out_layer.bias"] = u(256, sc=0.2) * flat
    sd["norm.weight"] = 1.0 + u(256, sc=0.3)
    sd["norm.bias"] = u(256, sc=0.2)
    sd["to_q.weight"] = u(inner, 256, sc=(3.0 / 256) ** 0.5)
    if lu_dim:
        sd["lu.weight"] = u(lu_dim, lu_dim, sc=(3.0 / lu_dim) ** 0.5)
        sd["lu.bias"] = u(lu_dim, sc=0.2)
    return sd


def make_input(rows, width, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(rows, width, generator=g) * 2 - 1) * 2.0


def _n_mid(sd):
    n = 0
    while f"net.layers.{n}.weight" in sd:
        n += 1
    return n


def chain(x, sd, act, dtype):
    """(q, h): the chain in `dtype` as plain torch calls -- oracle.flow_oracle.mlp, then the query side of cross_attention times I^-0.5 log2 e;
    h = the out_layer's output, in front of LayerNorm.  With lu.* in sd, x is the previous latent and the chain reads the first k_in columns
    of lu(x)."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    f = ACTS[act]
    if "lu.weight" in sd:
        x = F.linear(x, sd["lu.weight"], sd["lu.bias"])
    x = x[:, :sd["net.in_layer.weight"].shape[1]]
    x = f(F.linear(x, sd["net.in_layer.weight"], sd["net.in_layer.bias"]))
    keep = None
    for i in range(_n_mid(sd)):
        y = F.linear(x, sd[f"net.layers.{i}.weight"], sd[f"net.layers.{i}.bias"])
        if i % 2 == 0:
            keep = x
            x = f(y)
        else:
            x = f(keep + y)
    h = F.linear(x, sd["net.out_layer.weight"], sd["net.out_layer.bias"])
    hn = F.layer_norm(h, (h.shape[-1],), sd["norm.weight"], sd["norm.bias"], 1e-5)
    inner = sd["to_q.weight"].shape[0]
    return hn @ sd["to_q.weight"].t() * (inner ** -0.5 * LOG2E), h


def q_ref64(x, sd, act):
    return chain(x, sd, act, torch.float64)


def restated32(x, sd, act, fault=None):
    """The chain written out in fp32 (own LayerNorm: mean, biased variance, eps 1e-5), which can carry ONE planted fault of FAULTS."""
    assert fault is None or fault in FAULTS
    sd = {k: v.float() for k, v in sd.items()}
    f = ACTS[act]
    if fault == "tanh_gelu":
        assert act == "gelu"
        f = lambda t: F.gelu(t, approximate="tanh")
    rnd = (lambda t: t.half().float()) if fault == "fp16_acts" else (lambda t: t)      # a lost low limb
    x = rnd(x.float()[:, :sd["net.in_layer.weight"].shape[1]])
    x = rnd(f(x @ sd["net.in_layer.weight"].t() + sd["net.in_layer.bias"]))
    h_in = x
    h0 = rnd(f(x @ sd["net.layers.0.weight"].t() + sd["net.layers.0.bias"]))
    keep = h0 if fault == "residual_from_hidden0" else h_in
    h1 = rnd(f(keep + (h0 @ sd["net.layers.1.weight"].t() + sd["net.layers.1.bias"])))
    h = rnd(h1 @ sd["net.out_layer.weight"].t() + sd["net.out_layer.bias"])
    mean = h.mean(-1, keepdim=True)
    dlt = h - mean
    var = (dlt * dlt).sum(-1, keepdim=True) / (255.0 if fault == "var_over_255" else 256.0)
    n = rnd(dlt / torch.sqrt(var + (1e-6 if fault == "eps_1e-6" else 1e-5)))
    hn = n * sd["norm.weight"] + sd["norm.bias"]
    inner = sd["to_q.weight"].shape[0]
    return hn @ sd["to_q.weight"].t() * (inner ** -0.5 * LOG2E)


class Case:
    """One seeded problem with its references, computed once: x, sd, q64 (fp64), e32 = max |fp32 chain - q64|, row_std_min."""

    def __init__(self, k_in, rows, act, family, inner, lu_dim, seed):
        self.k_in, self.rows, self.act, self.family, self.inner, self.lu_dim = k_in, rows, act, family, inner, lu_dim
        self.sd = make_state(k_in, seed, inner=inner, family=family, lu_dim=lu_dim)
        self.x = make_input(rows, lu_dim if lu_dim else k_in, seed + 1000)         # with a pre-layer: the previous latent xprev [rows, D]
        self.q64, h = q_ref64(self.x, self.sd, act)
        self.e32 = (chain(self.x, self.sd, act, torch.float32)[0].double() - self.q64).abs().max().item()
        self.row_std_min = h.std(-1, unbiased=False).min().item()
        if lu_dim:
            self.xnext64 = F.linear(self.x.double(), self.sd["lu.weight"].double(), self.sd["lu.bias"].double())

    def label(self):
        return (f"k_in {self.k_in} (K_pad {math.ceil(self.k_in / 32) * 32}) rows {self.rows} {self.act} {self.family} I {self.inner}"
                + (f" pre-layer D {self.lu_dim}" if self.lu_dim else ""))

    def ratio(self, q):
        """max |q - q64| / e32, after the checks every case makes on its reference."""
        assert self.row_std_min > MIN_ROW_STD, f"{self.label()}: ill-conditioned LayerNorm input, min row std {self.row_std_min:.2e}"
        assert tuple(q.shape) == tuple(self.q64.shape), (tuple(q.shape), tuple(self.q64.shape))
        assert torch.isfinite(q).all()
        return (q.double().cpu() - self.q64).abs().max().item() / self.e32


@functools.lru_cache(maxsize=None)
def case(k_in, rows=300, act="gelu", family="plain", inner=64, lu_dim=0):
    seed = 7 + k_in * 13 + rows * 101 + ACT_NAMES.index(act) * 1009 + (5003 if family == "flat" else 0) + inner * 3 + lu_dim * 17
    return Case(k_in, rows, act, family, inner, lu_dim, seed)


WIDTHS = (20, 64, 90, 100, 132, 150, 190, 224, 256)          # K_pad 32, 64, 96, 128, 160, 160, 192, 224, 256
FAMILIES = ("plain", "flat")
