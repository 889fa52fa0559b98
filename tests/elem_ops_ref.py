"""Plain differentiable torch references of the flow's per-point training closures (csrc/train_rows.hip: affine coupling, the augmenter's
Gaussian draw, the Slice log-density, the base density; csrc/train_expm.hip: ExponentialCoupling at d2 <= 16) and of the stand-alone activation passes
(csrc/train_linear.hip), the inputs of their operator tests and the narrow ExponentialCoupling gate.  Everything works on dense [rows, c] tensors
in whatever dtype it is given: fp64 is the reference, the same function in eager fp32 on the CPU is the yardstick
(tests/test_gpu_train_elem_ops.py, with embed_ops_ref.gate).  Written from the formulae in the kernel headers;
tests/test_oracle_elem_ops.py pins every function to oracle/ on the CPU."""
import functools
import math

import torch

from embed_ops_ref import gate, rel  # noqa: F401  (the gate the operator tests share)
from test_expm_wide_bwd_host import autograd_reference, make_case, make_w  # noqa: F401

HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


# ---------------------------------------------------------------- references
def affine_ref(x2, st, d2, kind):
    """st = [raw scale d2 | shift d2] -> (y2 = x2 s + t, ldj = sum log s); s = exp(raw) or (2 sigmoid(raw) - 1)(1 - 1e-8) + 1."""
    raw, t = st[:, :d2], st[:, d2:2 * d2]
    if kind == "exp":
        s = torch.exp(raw)
    elif kind == "sigmoid":
        s = (2 * torch.sigmoid(raw) - 1) * (1 - 1e-8) + 1
    else:
        raise ValueError(kind)
    return x2 * s + t, torch.log(s).sum(-1)


def _std(p, nz, clamp):
    std = torch.exp(p[:, nz:2 * nz])
    return std.clamp_max(clamp) if clamp > 0 else std


def gauss_draw_ref(p, eps, nz, clamp):
    """p = [mean nz | log std nz] -> (z = mean + eps std, ldj = sum (eps^2 / 2 + log std + log(2 pi) / 2)); std = min(exp(log std), clamp)
    when clamp > 0."""
    std = _std(p, nz, clamp)
    return p[:, :nz] + eps * std, (0.5 * eps ** 2 + torch.log(std) + HALF_LOG_2PI).sum(-1)


def normal_log_prob_ref(v, p, nz, clamp):
    """sum_j log N(v_j; mean_j, std_j) per row, std as in `gauss_draw_ref`."""
    std = _std(p, nz, clamp)
    d = (v[:, :nz] - p[:, :nz]) / std
    return (-0.5 * d ** 2 - torch.log(std) - HALF_LOG_2PI).sum(-1)


def base_density_ref(x):
    return (-0.5 * x ** 2 - HALF_LOG_2PI).sum(-1)


def act_ref(u, name):
    """models/nets.py: GELU (exact erf form), RELU, ELU (alpha 1)."""
    if name == "GELU":
        return 0.5 * u * (1 + torch.erf(u / math.sqrt(2.0)))
    if name == "RELU":
        return torch.where(u > 0, u, torch.zeros_like(u))
    if name == "ELU":
        return torch.where(u > 0, u, torch.expm1(u))
    raise ValueError(name)


def run_ref(fn, inputs, weights, dtype, frozen=()):
    """fn(**inputs) -> dict of outputs, in `dtype` on the CPU; L = sum_k sum(out_k weights_k).  Returns the outputs and "d<name>" for every
    floating input that is not `frozen`."""
    x = {k: v.detach().to(dtype).clone().requires_grad_(k not in frozen) for k, v in inputs.items()}
    out = fn(**x)
    sum((out[k] * w.to(dtype)).sum() for k, w in weights.items()).backward()
    r = {k: v.detach() for k, v in out.items()}
    r.update({"d" + k: v.grad for k, v in x.items() if k not in frozen})
    return r


# ---------------------------------------------------------------- ExponentialCoupling, d2 <= 16 (expm_train_fwd_kernel / expm_train_bwd_kernel)
def expm_w(raw, scal4, dtype):
    """W = rescale tanh(scale raw + shift) + reshift + 1e-8 in `dtype`."""
    s4 = scal4.to(dtype)
    return s4[2] * torch.tanh(s4[0] * raw.to(dtype) + s4[1]) + s4[3] + 1e-8


def narrow_recurrence_backward(W, x, dy):
    """What the narrow kernels do, in W's dtype, for one point (W [d2, d2], x, dy [d2]) or a batch ([n, d2, d2], [n, d2]): per point
    s = the smallest s <= 6 with |W|_inf 2^-s <= 1/2, 2^s repetitions of the 12-term Taylor action v <- sum_k t_k, t_0 = v,
    t_k = (2^-s / k) W t_{k-1}, then exact reverse mode with s constant: mu_12 = lambda, dW += (2^-s / k) mu_k t_{k-1}^T,
    mu_{k-1} = lambda + (2^-s / k) W^T mu_k.  Returns (y - b, dx, dW, s); s an int, or an int64 tensor [n] for a batch."""
    if W.dim() == 2:
        y, dx, dW, s = narrow_recurrence_backward(W[None], x[None], dy[None])
        return y[0], dx[0], dW[0], int(s[0])
    nrm = W.abs().sum(-1).max(-1).values
    s = torch.zeros(W.shape[0], dtype=torch.int64)
    for _ in range(6):
        big = nrm > 0.5
        nrm = torch.where(big, nrm * 0.5, nrm)
        s += big
    y, dx, dW = torch.empty_like(x), torch.empty_like(x), torch.empty_like(W)
    for sv in s.unique().tolist():
        pick = s == sv
        Wp, f = W[pick], 2.0 ** -sv
        mv = lambda A, t: torch.einsum("nij,nj->ni", A, t)
        states = [x[pick]]
        for _ in range(1 << sv):
            acc = term = states[-1]
            for k in range(1, 13):
                term = mv(Wp, term) * (f / k)
                acc = acc + term
            states.append(acc)
        lam, g = dy[pick], torch.zeros_like(Wp)
        WT = Wp.transpose(1, 2)
        for v in reversed(states[:-1]):
            terms = [v]
            for k in range(1, 13):
                terms.append(mv(Wp, terms[-1]) * (f / k))
            mu = lam
            for k in range(12, 0, -1):
                mi = mu * (f / k)
                g = g + mi[:, :, None] * terms[k - 1][:, None, :]
                mu = lam + mv(WT, mi)
            lam = mu
        y[pick], dx[pick], dW[pick] = states[-1], lam, g
    return y, dx, dW, s


# name -> d2, ||W||_1 (test_expm_wide_bwd_host.make_w), rows, seed.  The norms give s = 0 (0.01) up to 5 or 6 (16.0); 70 rows cross a
# 64-point block.  Seeds: the first of 0, 1, 2, ... at which every row has |W|_inf <= 0.9 * 32 (tests/test_oracle_elem_ops.py checks it).
EXPM_CASES = {
    "x1_n001_r5": dict(d2=1, norm=0.01, rows=5, seed=0),
    "x1_n16_r70": dict(d2=1, norm=16.0, rows=70, seed=0),
    "x3_n03_r70": dict(d2=3, norm=0.3, rows=70, seed=0),
    "x3_n4_r5": dict(d2=3, norm=4.0, rows=5, seed=0),
    "x8_n001_r70": dict(d2=8, norm=0.01, rows=70, seed=0),
    "x8_n16_r5": dict(d2=8, norm=16.0, rows=5, seed=0),
    "x15_n03_r5": dict(d2=15, norm=0.3, rows=5, seed=0),
    "x15_n4_r70": dict(d2=15, norm=4.0, rows=70, seed=0),
    "x16_n001_r5": dict(d2=16, norm=0.01, rows=5, seed=0),
    "x16_n4_r5": dict(d2=16, norm=4.0, rows=5, seed=0),
    "x16_n16_r70": dict(d2=16, norm=16.0, rows=70, seed=0),
}
EXPM_BOUND_CASE = dict(d2=8, norm=100.0, rows=5, seed=0)           # every row beyond |W|_inf = 32: the status word, no result
EXPM_NORM_LIMIT = 32.0


def make_expm_case(name):
    c = dict(EXPM_BOUND_CASE if name == "bound" else EXPM_CASES[name])
    keys = ("raw", "x2", "b", "dy2", "dldj", "scal4")
    c.update(zip(keys, make_case(c["d2"], c["norm"], c["rows"], c["seed"])))
    return c


def expm_refs(c, dtype):
    """autograd_reference (fp64 / eager fp32 through torch.matrix_exp) plus ldj = tr W."""
    r = autograd_reference(c["raw"], c["x2"], c["b"], c["dy2"], c["dldj"], c["scal4"], dtype)
    r["ldj"] = torch.diagonal(expm_w(c["raw"], c["scal4"], dtype), dim1=1, dim2=2).sum(-1)
    return r


def _rel0(a, b):
    return rel(a, b, floor=0.0)


@functools.lru_cache(maxsize=None)
def narrow_yardstick():
    """name -> (err y, err dx, err dW, min s, max s) of `narrow_recurrence_backward` in fp32 against fp64 autograd through
    torch.matrix_exp, on the W the kernel sees (the fp32 W of every committed case), per tensor as max |a - a64| / max |a64|."""
    out = {}
    for name in EXPM_CASES:
        c = make_expm_case(name)
        W32 = expm_w(c["raw"], c["scal4"], torch.float32)
        W64, x64 = W32.double().requires_grad_(True), c["x2"].double().requires_grad_(True)
        y64 = torch.einsum("rij,rj->ri", torch.matrix_exp(W64), x64)
        (y64 * c["dy2"].double()).sum().backward()
        y, dx, dW, s = narrow_recurrence_backward(W32, c["x2"], c["dy2"])
        out[name] = (_rel0(y, y64.detach()), _rel0(dx, x64.grad), _rel0(dW, W64.grad), int(s.min()), int(s.max()))
    return out


def expm_gate():
    """The gate of y2, dx2 and the d raw block of the narrow kernels: max(2e-6, 3 x the largest error of the fp32 restatement).  2e-6: the
    gate of the wide operator (tests/test_gpu_expm_wide_bwd.py); 3: the margin for another summation order and tanhf."""
    return max(2e-6, 3 * max(max(v[:3]) for v in narrow_yardstick().values()))


# ---------------------------------------------------------------- inputs of the row-kernel tests
# Common: rows 1, 257 (rows_pad 512), 300; widths 3, 32 (no pad column), 150 (the shipped half-latent), 300 (second trip of the 256-stride
# loop).  wide: every input panel is 32 columns wider than it needs to be, and those columns hold other data (the backward then takes
# the zeros_like path); junk: the pad rows of every input panel and upstream gradient hold junk.
# high=False: no entry at +8.  With exp, s = e^8 at such an entry sets max |y2| and max |d scale| near 1e4, and the gate, relative to
# that maximum, then sees an error on an ordinary entry only from about 0.05 on; the one exp case without them keeps the gate at the
# scale of the ordinary entries (raw scale at most 3, s <= e^3; the entries at -8 stay).
AFFINE_CASES = {
    "a300_d150_sigmoid": dict(rows=300, d2=150, kind="sigmoid", wide=False, junk=0.0, seed=0),
    "a257_d300_exp": dict(rows=257, d2=300, kind="exp", wide=False, junk=7.0, seed=1),
    "a1_d3_exp": dict(rows=1, d2=3, kind="exp", wide=False, junk=0.0, seed=2),
    "a300_d32_sigmoid": dict(rows=300, d2=32, kind="sigmoid", wide=False, junk=7.0, seed=3),
    "a257_d150_exp_wide": dict(rows=257, d2=150, kind="exp", wide=True, junk=7.0, seed=4),
    "a300_d3_sigmoid_wide": dict(rows=300, d2=3, kind="sigmoid", wide=True, junk=0.0, seed=5),
    "a1_d300_sigmoid_wide": dict(rows=1, d2=300, kind="sigmoid", wide=True, junk=7.0, seed=6),
    "a300_d150_exp_low": dict(rows=300, d2=150, kind="exp", wide=False, junk=0.0, seed=7, high=False),
}
SATURATED = 8.0


def make_affine_case(name):
    """raw scale 1.5 N(0, 1) with every 11th entry and the last one +-8 (the sigmoid saturates, log s stays finite), x2, shift, dy2, dldj ~ N(0, 1);
    high=False: -8 only, and the draw itself kept below 3."""
    c = dict(AFFINE_CASES[name])
    g = torch.Generator().manual_seed(c["seed"])
    rows, d2 = c["rows"], c["d2"]
    raw = 1.5 * torch.randn(rows * d2, generator=g)
    if c.get("high", True):
        raw[::11] = SATURATED
    else:
        raw.clamp_(max=3.0)
    raw[5::22] = -SATURATED
    raw[-1] = -SATURATED
    c["x2"] = torch.randn(rows, d2, generator=g)
    c["st"] = torch.cat((raw.view(rows, d2), torch.randn(rows, d2, generator=g)), 1)
    c["dy2"], c["dldj"] = torch.randn(rows, d2, generator=g), torch.randn(rows, generator=g)
    return c


def affine_refs(c, dtype):
    d2 = c["d2"]
    fn = lambda x2, st: dict(zip(("y2", "ldj"), affine_ref(x2, st, d2, c["kind"])))
    r = run_ref(fn, dict(x2=c["x2"], st=c["st"]), dict(y2=c["dy2"], ldj=c["dldj"]), dtype)
    r["dscale"], r["dshift"] = r["dst"][:, :d2], r["dst"][:, d2:]
    del r["dst"]
    return r


# clamp 0: none; 10.0: the default clamp_dist; 0.5: below 1, so log(clamp) < 0
GAUSS_CASES = {
    "g300_n150_c10": dict(rows=300, nz=150, clamp=10.0, wide=False, junk=0.0, seed=0),
    "g257_n300_c05": dict(rows=257, nz=300, clamp=0.5, wide=False, junk=7.0, seed=1),
    "g1_n3_c10": dict(rows=1, nz=3, clamp=10.0, wide=False, junk=0.0, seed=2),
    "g300_n32_c0": dict(rows=300, nz=32, clamp=0.0, wide=False, junk=7.0, seed=3),
    "g257_n150_c10_wide": dict(rows=257, nz=150, clamp=10.0, wide=True, junk=7.0, seed=4),
    "g300_n3_c05_wide": dict(rows=300, nz=3, clamp=0.5, wide=True, junk=0.0, seed=5),
    "g1_n300_c0_wide": dict(rows=1, nz=300, clamp=0.0, wide=True, junk=7.0, seed=6),
}
NORMLP_CASES = {
    "l300_n150_c10": dict(rows=300, nz=150, clamp=10.0, wide=False, wide_v=False, junk=0.0, seed=10),
    "l257_n300_c05": dict(rows=257, nz=300, clamp=0.5, wide=False, wide_v=False, junk=7.0, seed=11),
    "l1_n3_c05": dict(rows=1, nz=3, clamp=0.5, wide=False, wide_v=False, junk=0.0, seed=12),
    "l300_n32_c0": dict(rows=300, nz=32, clamp=0.0, wide=False, wide_v=False, junk=7.0, seed=13),
    "l257_n150_c10_wide_v": dict(rows=257, nz=150, clamp=10.0, wide=False, wide_v=True, junk=7.0, seed=14),
    "l300_n3_c10_wide": dict(rows=300, nz=3, clamp=10.0, wide=True, wide_v=True, junk=0.0, seed=15),
    "l1_n300_c0_wide": dict(rows=1, nz=300, clamp=0.0, wide=True, wide_v=False, junk=7.0, seed=16),
}
CLAMP_MARGIN = 1e-3          # every log std at least this far from log(clamp): expf(ls) > clamp cannot disagree with the reference's compare
CLAMP_SHARE = 0.25           # ... and at least this share of the entries on either side


def clamp_cases():
    """(table name, case name) of every committed case with a clamp."""
    return [(t, n) for t, tab in (("gauss", GAUSS_CASES), ("normlp", NORMLP_CASES)) for n, c in tab.items() if c["clamp"] > 0]


def _log_std(g, rows, nz, clamp):
    """fp32 [rows, nz].  clamp == 0: 0.7 N(0, 1) - 0.3.  Otherwise log(clamp) +- (1.5 margin + 0.7 |N(0, 1)|), every 7th entry at 1.5 margin
    exactly; the side is a coin per entry, after a quarter of the entries (rounded up) was dealt to each side."""
    n = rows * nz
    if clamp <= 0:
        return (0.7 * torch.randn(n, generator=g) - 0.3).view(rows, nz)
    q = -(-n // 4)
    above = torch.rand(n, generator=g) < 0.5
    perm = torch.randperm(n, generator=g)
    above[perm[:q]] = True
    above[perm[q:2 * q]] = False
    dist = 1.5 * CLAMP_MARGIN + 0.7 * torch.randn(n, generator=g, dtype=torch.float64).abs()
    dist[::7] = 1.5 * CLAMP_MARGIN
    return (math.log(clamp) + torch.where(above, dist, -dist)).float().view(rows, nz)


def clamp_margins(c):
    """(min |log std - log clamp|, share above, share below) of a case's fp32 log std, in fp64."""
    nz = c["nz"]
    d = c["p"][:, nz:].double() - math.log(c["clamp"])
    return d.abs().min().item(), (d > 0).double().mean().item(), (d < 0).double().mean().item()


def make_gauss_case(name):
    c = dict(GAUSS_CASES[name])
    g = torch.Generator().manual_seed(c["seed"])
    rows, nz = c["rows"], c["nz"]
    c["p"] = torch.cat((torch.randn(rows, nz, generator=g), _log_std(g, rows, nz, c["clamp"])), 1)
    c["eps"] = torch.randn(rows, nz, generator=g)
    c["dz"], c["dldj"] = torch.randn(rows, nz, generator=g), torch.randn(rows, generator=g)
    return c


def _split_dp(r, nz):
    r["dmean"], r["dlogstd"] = r["dp"][:, :nz], r["dp"][:, nz:]
    del r["dp"]
    return r


def gauss_refs(c, dtype):
    nz = c["nz"]
    fn = lambda p, eps: dict(zip(("z", "ldj"), gauss_draw_ref(p, eps, nz, c["clamp"])))
    return _split_dp(run_ref(fn, dict(p=c["p"], eps=c["eps"]), dict(z=c["dz"], ldj=c["dldj"]), dtype, frozen=("eps",)), nz)


def make_normlp_case(name):
    """v a few std from the mean: mean + 2.5 N(0, 1) std, std the clamped one."""
    c = dict(NORMLP_CASES[name])
    g = torch.Generator().manual_seed(c["seed"])
    rows, nz = c["rows"], c["nz"]
    c["p"] = torch.cat((torch.randn(rows, nz, generator=g), _log_std(g, rows, nz, c["clamp"])), 1)
    c["v"] = c["p"][:, :nz] + 2.5 * torch.randn(rows, nz, generator=g) * _std(c["p"], nz, c["clamp"])
    c["g"] = torch.randn(rows, generator=g)
    return c


def normlp_refs(c, dtype):
    nz = c["nz"]
    fn = lambda v, p: dict(out=normal_log_prob_ref(v, p, nz, c["clamp"]))
    return _split_dp(run_ref(fn, dict(v=c["v"], p=c["p"]), dict(out=c["g"]), dtype), nz)


# scale: x ~ scale N(0, 1), or uniform on [-30, 30] for "u30" (the fp32 sum of x^2 / 2 reaches 4.5e4 over 300 columns)
BASE_CASES = {
    "b300_w150": dict(rows=300, width=150, wide=False, junk=0.0, scale=1.0, seed=20),
    "b257_w300": dict(rows=257, width=300, wide=False, junk=7.0, scale=1.0, seed=21),
    "b1_w3": dict(rows=1, width=3, wide=False, junk=0.0, scale=1.0, seed=22),
    "b300_w32": dict(rows=300, width=32, wide=False, junk=7.0, scale=1.0, seed=23),
    "b257_w150_wide": dict(rows=257, width=150, wide=True, junk=7.0, scale=1.0, seed=24),
    "b300_w300_u30_wide": dict(rows=300, width=300, wide=True, junk=0.0, scale="u30", seed=25),
    "b1_w3_wide": dict(rows=1, width=3, wide=True, junk=7.0, scale=1.0, seed=26),
}


def make_base_case(name):
    c = dict(BASE_CASES[name])
    g = torch.Generator().manual_seed(c["seed"])
    rows, width = c["rows"], c["width"]
    c["x"] = (torch.rand(rows, width, generator=g) * 60 - 30) if c["scale"] == "u30" else c["scale"] * torch.randn(rows, width, generator=g)
    c["g"] = torch.randn(rows, generator=g)
    return c


def base_refs(c, dtype):
    return run_ref(lambda x: dict(out=base_density_ref(x)), dict(x=c["x"]), dict(out=c["g"]), dtype)
